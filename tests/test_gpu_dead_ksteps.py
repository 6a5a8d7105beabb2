"""Dead k-step skipping of the fp32 inference kernels (csrc/nerf_mlp_f32.hip.inc, gemm_tiles KSKIP; MlpArgs::skip_dead_ksteps):
a k-step whose activation register is zero in all 64 lanes issues no MFMAs.  `raw` must not change by a bit.

1. Switch on (default) against NERF_DEAD_KSTEP_SKIP=0, bit for bit, on every inference entry, on scenes whose CPU activations
   (oracle, fp32) are first shown to exercise the code: many dead k-steps, groups with a dead first row, groups with every row
   live ("base"), a scene with next to nothing to skip ("white"), and a network trained by the build itself.
2. Exact integer probes for the edges of the decision: weights, biases and inputs are small integers, every sum is exact in fp32
   in any order, and the expected `raw` is the float64 evaluation, compared exactly.  The positional encoding is routed through
   weights that read only the raw coordinate columns (sin / cos multiply zero weights)."""
import os
import sys

import pytest
import torch

from gpu_common import amd, network  # noqa: F401

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import dead_ksteps as dk  # noqa: E402  (the CPU probe: pairing and tile rule in one place)

RELU_FED = ("h0", "h1", "h2", "h3", "h4", "h5", "h6", "h7")


def _bits(x):
    return x.contiguous().view(torch.int32)


def _on_off(monkeypatch, run):
    """run() with the switch unset (skipping) and with NERF_DEAD_KSTEP_SKIP=0 (every MFMA issued) -> (on, off)."""
    monkeypatch.delenv("NERF_DEAD_KSTEP_SKIP", raising=False)
    on = run()
    monkeypatch.setenv("NERF_DEAD_KSTEP_SKIP", "0")
    off = run()
    monkeypatch.delenv("NERF_DEAD_KSTEP_SKIP")
    return on, off


# ------------------------------------------------------------------------------------------------ 1. switch on against switch off
_SCENES = {}


def _scene(oracle, family_sd, family):
    """64 seeded rays of the bench frame: the 64 coarse depths, the 192 sorted depths of the CPU oracle's fine_sample, and the CPU
    activations (fp32) of both passes cut into 32-sample tiles.  Computed once per family, never modified."""
    if family not in _SCENES:
        sd = family_sd(family)
        ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(0))[:64]
        o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(40.0), pixel_ids=ids)
        with torch.no_grad():
            _, _, parts = oracle.render(sd, o[None], d[None], return_parts=True)
        t_c, t_f, vd = parts["t_coarse"].contiguous(), parts["t_sorted"].contiguous(), parts["viewdirs"]
        acts = {}
        for key, prefix, t in (("coarse", "model", t_c), ("fine", "model_fine", t_f)):
            acts[key] = dk.tile_activations(sd, prefix, oracle.points_on_rays(o, d, t), vd)[1]
        _SCENES[family] = dict(sd=sd, o=o.contiguous(), d=d.contiguous(), t_c=t_c, t_f=t_f, acts=acts)
    return _SCENES[family]


def _dead_fractions(acts):
    return {k: dk.dead_ksteps(acts[k]).float().mean().item() for k in RELU_FED}


def _rays_forward(amd, fn, packed, o, d, t):
    n, S = t.shape
    raw = torch.full((n, S, 4), float("nan"), device="cuda")
    amd._lib.call(fn, o, d, t, S, n, S, packed, raw, 0)
    torch.cuda.synchronize()
    return raw


@pytest.mark.parametrize("family", ["base", "white", "trained"])
def test_switch_on_equals_switch_off(amd, oracle, family_sd, monkeypatch, family):
    """Every inference entry, 64 rays x 64 coarse depths (coarse model) and x 192 sorted depths (fine model), and 37 points (a
    ragged second tile): int32-equal with and without skipping.  Before any launch the CPU activations of the same points show
    what these inputs exercise."""
    sc = _scene(oracle, family_sd, family)
    fine, coarse = _dead_fractions(sc["acts"]["fine"]), _dead_fractions(sc["acts"]["coarse"])
    print(family, "fine", {k: round(v, 3) for k, v in fine.items()}, "coarse", {k: round(v, 3) for k, v in coarse.items()})
    if family == "base":
        assert min(fine.values()) >= 0.05, fine                             # (CPU figures of the bench frame: 17-30 %)
        groups = torch.cat([dk.dead_ksteps(sc["acts"]["fine"][k]).reshape(-1, 32, 4) for k in RELU_FED])     # [tiles, group, row]
        assert groups[..., 0].any(), "no group with a dead row 0: the loads-without-MFMAs path would not run"
        assert (~groups).all(-1).any(), "no group with all four rows live"
    if family == "white":
        assert min(fine.values()) < 0.02, fine                              # the path where nothing is skipped
    net = network(amd, sc["sd"], "f32", train=False)
    o, d = sc["o"].cuda(), sc["d"].cuda()
    for t, model in ((sc["t_c"], ""), (sc["t_f"], "fine")):
        t = t.cuda()
        for fn in ("nerf_mlp_forward_rays", "nerf_mlp_forward_rays_density", "nerf_mlp_forward_rays_for_compositing"):
            on, off = _on_off(monkeypatch, lambda: _rays_forward(amd, fn, net.packed(model), o, d, t))
            assert torch.isfinite(on).all() and on[..., 3].abs().max() > 0, (fn, model)
            assert torch.equal(_bits(on), _bits(off)), (family, fn, model)
    # points: the first 37 fine samples of ray 0 and their direction -- one full tile and 5 points of a second
    pts = oracle.points_on_rays(sc["o"][:1], sc["d"][:1], sc["t_f"][:1])[0, :37].reshape(37, 1, 3).contiguous().cuda()
    vd = (sc["d"][:1] / sc["d"][:1].norm(dim=-1, keepdim=True)).expand(37, 3).contiguous().cuda()

    def points():
        raw = torch.full((37, 1, 4), float("nan"), device="cuda")
        amd._lib.call("nerf_mlp_forward", pts, vd, 37, 1, net.packed("fine"), raw, 0)
        torch.cuda.synchronize()
        return raw
    on, off = _on_off(monkeypatch, points)
    assert torch.isfinite(on).all() and torch.equal(_bits(on), _bits(off)), family


def test_masked_pass_on_equals_off(amd, oracle, family_sd, monkeypatch):
    """The fine pass on a compacted index list (fast_sampling: only the samples that survive the ESS / ERT masks are evaluated, by
    id), with a list whose length is not a multiple of 32 -- the last tile is ragged and its padding lanes repeat the last id.
    The frame entry hands back rgb and depth; both are int32-equal with and without skipping."""
    sc = _scene(oracle, family_sd, "base")
    net = network(amd, sc["sd"], "f32", train=False)
    ren = amd.Renderer(net)
    L = amd._lib
    t_c, u = ren._get_tables(torch.device("cuda", torch.cuda.current_device()))

    def frame(n):
        o, d = sc["o"][:n].cuda().contiguous(), sc["d"][:n].cuda().contiguous()
        ws = torch.empty(int(L.call("nerf_render_occupancy_workspace_bytes", n, 128, 1)), dtype=torch.uint8, device="cuda")
        rgb, dep = torch.full((n, 3), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        evaluated = torch.zeros(2, dtype=torch.int64, device="cuda")
        L.call("nerf_render_forward_occupancy", o, d, n, net.packed(""), net.packed("fine"), t_c, u, 128, 1, 0, 1, 0.25,
               None, None, [1, 1, 1], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], evaluated, ws, ws.numel(), rgb, dep)
        torch.cuda.synchronize()
        return rgb, dep, int(evaluated[1].item())
    ragged = None
    for n in (61, 59, 53):                               # the first of these whose list is ragged (its length is the sampler's business)
        count = frame(n)[2]
        if 0 < count < n * 192 and count % 32 != 0:
            ragged = n
            break
    assert ragged is not None, "no ray count with a ragged index list"
    on, off = _on_off(monkeypatch, lambda: frame(ragged))
    assert on[2] == off[2] and on[2] % 32 != 0
    assert torch.isfinite(on[0]).all() and torch.isfinite(on[1]).all()
    assert torch.equal(_bits(on[0]), _bits(off[0])) and torch.equal(_bits(on[1]), _bits(off[1]))


# ------------------------------------------------------------------------------------------------ 2. exact integer probes
LAYERS = [f"pts_linears.{i}" for i in range(8)] + ["feature_linear", "views_linears.0", "alpha_linear", "rgb_linear"]


def _integer_sub(oracle, seed):
    """One sub-model of small integers: three +-1 weights per output (the encodings read through their raw-coordinate columns
    only), biases in [-1, 2].  Every partial sum of the network is an integer far below 2^24 (checked by _exact_bound)."""
    g = torch.Generator().manual_seed(seed)
    sub = {}
    for name in LAYERS:
        out_f, in_f = oracle.SUBMODEL_SHAPES[name + ".weight"]
        W = torch.zeros(out_f, in_f)
        cols = torch.arange(in_f)
        if name == "pts_linears.0":
            cols = torch.arange(3)                                          # x, y, z themselves
        elif name == "pts_linears.5":
            cols = torch.cat([torch.arange(3), torch.arange(63, 319)])
        elif name == "views_linears.0":
            cols = torch.cat([torch.arange(256), torch.arange(256, 259)])   # feature, and the raw direction
        for r in range(out_f):
            pick = cols[torch.randperm(len(cols), generator=g)[:3]]
            W[r, pick] = (torch.randint(0, 2, (3,), generator=g) * 2 - 1).float()
        sub[name + ".weight"] = W
        sub[name + ".bias"] = torch.randint(-1, 3, (out_f,), generator=g).float()
    return sub


def _sd_of(oracle, sub):
    sd = {f"{m}.{k}": v.clone() for m in ("model", "model_fine") for k, v in sub.items()}
    return {k: sd[k].contiguous() for k in oracle.state_dict_keys()}


def _exact_bound(sub, xmax):
    """The largest sum of absolute terms of any output of the network for |inputs| <= xmax, folded views layer included: below
    2^24 every such sum is exact in fp32 in any order."""
    A = lambda n: sub[n + ".weight"].abs().double()
    B = lambda n: sub[n + ".bias"].abs().double()
    pe = torch.zeros(63, dtype=torch.float64)
    pe[:3] = xmax                                                           # (the other columns only meet zero weights)
    h, worst = pe, 0.0
    for i in range(8):
        h = A(f"pts_linears.{i}") @ h + B(f"pts_linears.{i}")
        worst = max(worst, h.max().item())
        if i == 4:
            h = torch.cat([pe, h])
    dirs = torch.zeros(27, dtype=torch.float64)
    dirs[:3] = xmax
    Wv = A("views_linears.0")
    views = (Wv[:, :256] @ A("feature_linear")) @ h + Wv[:, 256:] @ dirs + (Wv[:, :256] @ B("feature_linear") + B("views_linears.0"))
    out = max((A("rgb_linear") @ views + B("rgb_linear")).max().item(), (A("alpha_linear") @ h + B("alpha_linear")).max().item())
    return max(worst, views.max().item(), out)


def _expected(oracle, sd, pts, dirs):
    """float64 evaluation of the fine model on points [P,3] with per-point directions [P,3] -> (raw [P,4] fp32, activations)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    emb = torch.cat([oracle.freq_encode(pts.double(), oracle.XYZ_FREQS), oracle.freq_encode(dirs.double(), oracle.DIR_FREQS)], -1)
    raw, acts = oracle.nerf_mlp(sd64, "model_fine", emb, return_activations=True)
    assert torch.equal(raw, raw.round()) and raw.abs().max() < 2 ** 24
    return raw.float(), acts


def _gpu_points(amd, net, pts, dirs):
    P = pts.shape[0]
    raw = torch.full((P, 1, 4), float("nan"), device="cuda")
    amd._lib.call("nerf_mlp_forward", pts.reshape(P, 1, 3).contiguous().cuda(), dirs.contiguous().cuda(), P, 1, net.packed("fine"), raw, 0)
    torch.cuda.synchronize()
    return raw.reshape(P, 4).cpu()


def _integer_points(P, seed):
    g = torch.Generator().manual_seed(100 + seed)
    return torch.randint(-2, 3, (P, 3), generator=g).float(), torch.randint(-2, 3, (P, 3), generator=g).float()


def _silence(sub, layer):
    """Layer `layer` (0..7) puts out nothing: zero weights on its ReLU-fed part and biases <= 0 (some of them 0)."""
    name = f"pts_linears.{layer}"
    sub[name + ".weight"].zero_()
    sub[name + ".bias"] = -(torch.arange(256) % 3).float()


def _check(amd, oracle, monkeypatch, sub, pts, dirs):
    """GPU == float64 reference exactly, with and without skipping (int32-equal to each other) -> (raw, activations)."""
    assert _exact_bound(sub, 3.0) < 2 ** 24
    sd = _sd_of(oracle, sub)
    want, acts = _expected(oracle, sd, pts, dirs)
    net = network(amd, sd, "f32", train=False)
    on, off = _on_off(monkeypatch, lambda: _gpu_points(amd, net, pts, dirs))
    assert torch.equal(_bits(on), _bits(off))
    assert torch.equal(on, want), (on - want).abs().max()
    return want, acts


@pytest.mark.parametrize("layer", [0, 4, 7])
def test_exact_whole_layer_dead(amd, oracle, monkeypatch, layer):
    """(a) Layer l's output is <= 0 at every point, so every k-step of the GEMM it feeds is dead, row 0 of every group included
    (its groups issue loads and no MFMA): the result is the image of that GEMM's biases.  l = 0; l = 4, the skip layer, whose
    positional-encoding part still runs; l = 7, which feeds the folded views GEMM (and leaves sigma = the head's bias).  One full
    tile and, in the same call, a ragged one (37 points)."""
    sub = _integer_sub(oracle, 7 + layer)
    _silence(sub, layer)
    pts, dirs = _integer_points(37, layer)
    want, acts = _check(amd, oracle, monkeypatch, sub, pts, dirs)
    assert acts[f"h{layer}"].abs().max() == 0
    if layer == 7:
        assert torch.all(want[:, 3] == sub["alpha_linear.bias"][0]) and acts["views"].abs().max() > 0
    else:
        assert acts[f"h{layer + 1}"].abs().max() > 0 and want.abs().max() > 0       # the biases' image went on through the network


@pytest.mark.parametrize("point,feature", [(0, 0), (31, 4), (0, 39), (31, 250)])
def test_exact_one_live_feature_in_one_point(amd, oracle, monkeypatch, point, feature):
    """(b) Layer 0 puts out exactly one positive value: feature f at one point of a 32-point tile -- lane 0 or lane 31 of its lane
    half (features with bit 2 clear live in lanes 0..31, their partners f + 4 in lanes 32..63), in the first row of a group
    (f & 3 == 0) and in a later one.  That k-step must run, alone in its layer, and its contribution must arrive."""
    sub = _integer_sub(oracle, 20)
    _silence(sub, 0)
    sub["pts_linears.0.weight"][feature, 0] = 1.0                           # relu(x - 2): positive where x = 3 only
    sub["pts_linears.0.bias"][feature] = -2.0
    sub["pts_linears.1.weight"][::5, feature] = 1.0                         # layer 1 reads it
    pts, dirs = _integer_points(32, 50 + feature)
    pts[point, 0] = 3.0
    want, acts = _check(amd, oracle, monkeypatch, sub, pts, dirs)
    h0 = acts["h0"]
    assert h0[point, feature] == 1 and h0.sum() == 1
    dead = dk.dead_ksteps(h0.reshape(1, 32, 256))[0]
    s = [i for i, (a, b) in enumerate(dk.kstep_pairs().tolist()) if feature in (a, b)]
    assert len(s) == 1 and not dead[s[0]] and dead.sum() == 127 and s[0] % 4 == (feature & 3)
    others = [p for p in range(32) if p != point]
    assert (acts["h1"][point] - torch.relu(sub["pts_linears.1.bias"].double())).abs().max() > 0       # the contribution
    assert torch.equal(acts["h1"][others], torch.relu(sub["pts_linears.1.bias"].double()).expand(31, 256))


@pytest.mark.parametrize("point", [36, 5])
def test_exact_ragged_tile(amd, oracle, monkeypatch, point):
    """(c) 37 points: the 27 padding lanes of the second tile repeat point 36 (the kernel clamps the point id), so a feature cannot
    be positive in padding lanes alone; what can happen is probed instead.  point = 36: the feature is positive at the last valid
    point only, i.e. in lane 4 of the ragged tile and in all of its padding lanes, and dead throughout the first tile.  point = 5:
    positive in the first tile only, and the ragged tile's row is dead in every lane, padding included.  The valid outputs
    equal the float64 result either way."""
    sub = _integer_sub(oracle, 21)
    _silence(sub, 0)
    sub["pts_linears.0.weight"][70, 1] = 1.0
    sub["pts_linears.0.bias"][70] = -2.0
    sub["pts_linears.1.weight"][::3, 70] = -1.0
    pts, dirs = _integer_points(37, 60)
    pts[point, 1] = 3.0
    want, acts = _check(amd, oracle, monkeypatch, sub, pts, dirs)
    assert acts["h0"][point, 70] == 1 and acts["h0"].sum() == 1
