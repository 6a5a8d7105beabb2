"""Leading dead groups of the fp32 inference kernels (csrc/nerf_mlp_f32.hip.inc, gemm_tiles `prefix`; MlpArgs::skip_dead_groups):
the run of all-dead 4-k-step groups a GEMM starts with is stepped over without a wait, a load or a row branch, and the first
group that runs fetches its own blocks.  A stepped-over group adds nothing to any accumulator, exactly as its four skipped rows
did before, so `raw` must not change by a bit: every comparison here is int32-equal.

1. Exact integer probes (the construction of tests/test_gpu_dead_ksteps.py: small-integer weights and inputs, expected `raw` from
   float64, compared exactly) that put a prefix of chosen length P in front of every consuming GEMM position (the group path
   exists in trunk layers 1-7; the folded views GEMM keeps the row path, see _CASES), on every inference
   entry (points, rays, density-only, for-compositing), in three settings: default, NERF_DEAD_GROUP_SKIP=0 (row decisions only)
   and NERF_DEAD_KSTEP_SKIP=0 (every MFMA issued).
2. The three settings against each other on real weights, ordered and identity streams, after the CPU activations under the same
   order have shown that the inputs exercise the path."""
import os
import sys

import pytest
import torch

import f16_reference as F
import unit_order_reference as U
from gpu_common import amd, network  # noqa: F401
from test_gpu_dead_ksteps import (_bits, _exact_bound, _expected, _integer_points, _integer_sub, _scene, _sd_of, _silence)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import dead_ksteps as dk  # noqa: E402

SETTINGS = ({}, {"NERF_DEAD_GROUP_SKIP": "0"}, {"NERF_DEAD_KSTEP_SKIP": "0"})
RAY_ENTRIES = ("nerf_mlp_forward_rays", "nerf_mlp_forward_rays_density", "nerf_mlp_forward_rays_for_compositing")


def _three(monkeypatch, run):
    """run() under the default (groups and rows skipped), with the group path off, and with all skipping off."""
    out = []
    for env in SETTINGS:
        for k in ("NERF_DEAD_GROUP_SKIP", "NERF_DEAD_KSTEP_SKIP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out.append(run())
    for k in ("NERF_DEAD_GROUP_SKIP", "NERF_DEAD_KSTEP_SKIP"):
        monkeypatch.delenv(k, raising=False)
    return out


# ------------------------------------------------------------------------------------------------ 1. exact integer probes
def _group_features(groups):
    """The features (of 256) held by the registers of the given groups of a GEMM's input."""
    pairs = dk.kstep_pairs()
    return sorted({int(f) for g in groups for s in range(4 * g, 4 * g + 4) for f in pairs[s].tolist()})


def _prefix(sub, layer, P):
    """Layer `layer` (0..7) puts out zero at every point on the features of its consumer's groups 0..P-1 (zero weights, biases
    <= 0) and, if P < 32, one on a feature of group P (zero weights, bias 1): the consumer's leading run is exactly P groups."""
    name = f"pts_linears.{layer}"
    if P >= 32:
        _silence(sub, layer)
        return
    dead = _group_features(range(P))
    sub[name + ".weight"][dead] = 0.0
    sub[name + ".bias"][dead] = -(torch.arange(len(dead)) % 3).float()
    live = _group_features([P])[1]
    sub[name + ".weight"][live] = 0.0
    sub[name + ".bias"][live] = 1.0


def _leading(acts, layer, tile=slice(None)):
    """Leading dead groups per 32-point tile of h<layer> ([P, 256], P a multiple of 32 or padded with its last point)."""
    h = acts[f"h{layer}"]
    pad = (-h.shape[0]) % 32
    if pad:
        h = torch.cat([h, h[-1:].expand(pad, 256)])
    return dk.dead_groups(dk.dead_ksteps(h.reshape(-1, 32, 256)))[1][tile].tolist()


def _probe_rays(n, S, seed):
    """n rays x S samples whose points are small integers: integer origins, +-unit axis directions, integer depths."""
    g = torch.Generator().manual_seed(900 + seed)
    o = torch.randint(-1, 2, (n, 3), generator=g).float()
    d = torch.zeros(n, 3)
    d[torch.arange(n), torch.randint(0, 3, (n,), generator=g)] = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    t = torch.randint(0, 3, (n, S), generator=g).float()
    return o, d, t


def _check_everywhere(amd, oracle, monkeypatch, sub, o, d, t, pts_override=None):
    """Every inference entry on the points o + d t (ray mode) and on the same points given explicitly, in the three settings,
    against the float64 evaluation, exactly.  pts_override [n*S, 3]: explicit points and per-point directions for the points
    entry only (then the ray entries are left out) -> (want, acts)."""
    assert _exact_bound(sub, 3.0) < 2 ** 24
    sd = _sd_of(oracle, sub)
    net = network(amd, sd, "f32", train=False)
    L = amd._lib
    if pts_override is None:
        n, S = t.shape
        pts = (o[:, None, :] + d[:, None, :] * t[..., None]).reshape(-1, 3)
        dirs = d[:, None, :].expand(n, S, 3).reshape(-1, 3)
    else:
        pts, dirs = pts_override
    assert pts.abs().max() <= 3
    P = pts.shape[0]
    want, acts = _expected(oracle, sd, pts, dirs)

    def points():
        raw = torch.full((P, 1, 4), float("nan"), device="cuda")
        L.call("nerf_mlp_forward", pts.reshape(P, 1, 3).contiguous().cuda(), dirs.contiguous().cuda(), P, 1, net.packed("fine"), raw, 0)
        torch.cuda.synchronize()
        return raw.reshape(P, 4).cpu()
    for got in _three(monkeypatch, points):
        assert torch.equal(got, want), (got - want).abs().max()
    if pts_override is not None:
        return want, acts
    live = (want[:, 3].reshape(-1, 32) > 0).any(-1).repeat_interleave(32) if P % 32 == 0 else None
    oc, dc, tc = o.contiguous().cuda(), d.contiguous().cuda(), t.contiguous().cuda()
    for fn in RAY_ENTRIES:
        def rays():
            raw = torch.full((n, S, 4), float("nan"), device="cuda")
            L.call(fn, oc, dc, tc, S, n, S, net.packed("fine"), raw, 0)
            torch.cuda.synchronize()
            return raw.reshape(P, 4).cpu()
        exp = want.clone()
        if fn.endswith("density"):
            exp[:, :3] = 0
        elif fn.endswith("compositing") and live is not None:
            exp[~live, :3] = 0                                              # a tile without a sigma > 0 skips the colour branch
        elif fn.endswith("compositing"):
            continue
        for got in _three(monkeypatch, rays):
            assert torch.equal(got, exp), (fn, (got - exp).abs().max())
    return want, acts


# consuming GEMM positions by the layer whose output they read: 0 -> the X->Y copy of the pair loop (layer 1), 1 -> the Y->X copy
# (layer 2), 4 -> layer 5 after its PE part, 6 -> layer 7 (full, DSKIP and density-only instances: the three ray entries),
# 7 -> the folded views GEMM.  The views GEMM (NT = 4, the non-spread form) has NO group path: it keeps the row decisions alone
# ("Leading dead groups").  Its cases, P = 3, 4, 5 for every slot phase included, therefore prove nothing
# about the new code; they stay as the exact pins of that position that a later change giving it a prefix has to keep, and they
# show that the switch leaves it alone.
_CASES = [(l, P) for l in (0, 1, 4, 6, 7) for P in (0, 1, 2, 15, 30, 31, 32)] + [(7, 3), (7, 4), (7, 5)]


@pytest.mark.parametrize("layer,P", _CASES)
def test_exact_prefix_of_every_length_at_every_position(amd, oracle, monkeypatch, layer, P):
    """The first P groups of the input are dead in every lane and group P is live.  Two rays x 32 samples: two full tiles."""
    sub = _integer_sub(oracle, 300 + layer)
    _prefix(sub, layer, P)
    o, d, t = _probe_rays(2, 32, 10 * layer + P)
    want, acts = _check_everywhere(amd, oracle, monkeypatch, sub, o, d, t)
    assert _leading(acts, layer) == [P, P]
    assert want.abs().max() > 0
    if layer == 6:
        assert (want[:, 3] > 0).any() or P == 32                            # (a live tile: the full instance's colour branch ran)


@pytest.mark.parametrize("P", [5, 6])
@pytest.mark.parametrize("point,half", [(0, 0), (31, 0), (0, 1), (31, 1)])
def test_exact_group_live_in_its_last_row_at_one_point(amd, oracle, monkeypatch, P, point, half):
    """Layer 0 puts out exactly one positive value: a feature of the LAST row of group P, at point 0 or 31 of the tile -- lane 0
    or 31 of the lane half that holds the feature.  Groups 0..P-1 are the prefix (both slot parities), group P must be fetched
    and run, and every group behind it is dead again (today's path)."""
    sub = _integer_sub(oracle, 320)
    _silence(sub, 0)
    feature = int(dk.kstep_pairs()[4 * P + 3][half])
    sub["pts_linears.0.weight"][feature, 0] = 1.0                           # relu(x - 2): positive where x = 3 only
    sub["pts_linears.0.bias"][feature] = -2.0
    sub["pts_linears.1.weight"][::5, feature] = 1.0
    pts, dirs = _integer_points(32, 70 + P)
    pts[point, 0] = 3.0
    want, acts = _check_everywhere(amd, oracle, monkeypatch, sub, None, None, None, pts_override=(pts, dirs))
    assert acts["h0"][point, feature] == 1 and acts["h0"].sum() == 1
    assert _leading(acts, 0) == [P]
    assert (acts["h1"][point] - torch.relu(sub["pts_linears.1.bias"].double())).abs().max() > 0       # the contribution arrived


def test_exact_two_tiles_with_different_prefixes(amd, oracle, monkeypatch):
    """One launch, two tiles: the first leaves its prefix at group 3, the second at group 10."""
    sub = _integer_sub(oracle, 330)
    _silence(sub, 0)
    f1, f2 = _group_features([3])[0], _group_features([10])[2]
    for f, axis in ((f1, 0), (f2, 1)):
        sub["pts_linears.0.weight"][f, axis] = 1.0
        sub["pts_linears.0.bias"][f] = -2.0
        sub["pts_linears.1.weight"][::7, f] = 1.0
    pts, dirs = _integer_points(64, 80)
    pts[5, 0] = 3.0
    pts[40, 1] = 3.0
    want, acts = _check_everywhere(amd, oracle, monkeypatch, sub, None, None, None, pts_override=(pts, dirs))
    assert _leading(acts, 0) == [3, 10]


def test_exact_one_tile_with_different_prefixes_in_consecutive_layers(amd, oracle, monkeypatch):
    sub = _integer_sub(oracle, 340)
    for layer, P in ((0, 4), (1, 9), (2, 1), (3, 31)):
        _prefix(sub, layer, P)
    o, d, t = _probe_rays(1, 32, 90)
    want, acts = _check_everywhere(amd, oracle, monkeypatch, sub, o, d, t)
    assert [_leading(acts, l)[0] for l in range(4)] == [4, 9, 1, 31]


def test_exact_ragged_tile_whose_padding_keeps_group_0_alive(amd, oracle, monkeypatch):
    """37 points: the only positive value of layer 0 sits in group 0 at the last valid point, which the 27 padding lanes of the
    second tile repeat.  The first tile's input is wholly dead (its prefix ends at the last group, which always runs); the ragged
    tile has no prefix."""
    sub = _integer_sub(oracle, 350)
    _silence(sub, 0)
    f = _group_features([0])[3]
    sub["pts_linears.0.weight"][f, 1] = 1.0
    sub["pts_linears.0.bias"][f] = -2.0
    sub["pts_linears.1.weight"][::3, f] = -1.0
    pts, dirs = _integer_points(37, 95)
    pts[36, 1] = 3.0
    want, acts = _check_everywhere(amd, oracle, monkeypatch, sub, None, None, None, pts_override=(pts, dirs))
    assert acts["h0"][36, f] == 1 and acts["h0"].sum() == 1
    assert _leading(acts, 0) == [32, 0]


@pytest.mark.parametrize("seed,zero_axis", [(0, 0), (1, 2)])
def test_masked_list_three_settings(amd, monkeypatch, seed, zero_axis):
    """The coarse-only culled frame of tests/test_gpu_unit_order.py::test_integer_probes_masked_list (an inference launch on a
    compacted index list, ragged lists among them), on a probe network whose layers 1 and 3 carry dead prefixes of 6 and 11
    groups: rgb, depth and the number of evaluated samples are int32-equal in the three settings.  This compares the settings
    with each other, not with a float64 reference: the all-off setting runs code this change does not touch, and that code is
    held to the reference by the test named above; a defect shared by the row path and the group path is what the float64
    probes above are for."""
    L = amd._lib
    sd = F.both_models(F.probe_network(seed, zero_axis))
    for layer, P in ((1, 6), (3, 11)):
        dead = _group_features(range(P))
        for m in ("model", "model_fine"):
            sd[f"{m}.pts_linears.{layer}.weight"][dead] = 0.0
            sd[f"{m}.pts_linears.{layer}.bias"][dead] = 0.0
    sd = {k: v.contiguous() for k, v in sd.items()}
    net = network(amd, sd, "f32")
    gen = torch.Generator().manual_seed(6000 + seed)
    o_all, _, _, _, unit = F.probe_rays(gen, zero_axis, 65, 1, per_ray=False)
    o_all, d_all = (o_all - 2.0 * unit).contiguous(), unit.contiguous()
    t_c = (2.0 + torch.arange(64, dtype=torch.float32) / 16).cuda()
    u = torch.linspace(0.0, 1.0, 128).cuda()
    words = int(L.call("nerf_occupancy_words", 17, 17, 17))
    bits = torch.randint(-2 ** 31, 2 ** 31, (words,), generator=gen, dtype=torch.int64).to(torch.int32).cuda()

    def frame(n):
        o, d = o_all[:n].cuda().contiguous(), d_all[:n].cuda().contiguous()
        ws = torch.empty(int(L.call("nerf_render_occupancy_workspace_bytes", n, 0, 0)), dtype=torch.uint8, device="cuda")
        rgb, dep = torch.full((n, 3), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        evaluated = torch.zeros(2, dtype=torch.int64, device="cuda")
        L.call("nerf_render_forward_occupancy", o, d, n, net.packed_inference(""), None, t_c, u, 0, 1, 0, 0, 0.0,
               bits, None, [17, 17, 17], [-8.0, -8.0, -8.0], [1.0, 1.0, 1.0], evaluated, ws, ws.numel(), rgb, dep)
        torch.cuda.synchronize()
        return rgb, dep, int(evaluated[0].item())
    ragged = False
    for n in (1, 31, 33, 65):
        on, rows, off = _three(monkeypatch, lambda: frame(n))
        assert torch.isfinite(on[0]).all() and torch.isfinite(on[1]).all() and 0 < on[2] < 64 * n
        ragged = ragged or on[2] % 32 != 0
        for other in (rows, off):
            assert other[2] == on[2] and torch.equal(_bits(other[0]), _bits(on[0])) and torch.equal(_bits(other[1]), _bits(on[1])), n
    assert ragged


# ------------------------------------------------------------------------------------------------ 2. the three settings, real weights
RELU_FED = ("h0", "h1", "h2", "h3", "h4", "h5", "h6", "h7")


def _ordered_leading(acts, order):
    """{h: (all-dead groups, leading run) per tile} of CPU activations under a unit order [8, 256]."""
    out = {}
    for l, h in enumerate(RELU_FED):
        n, lead, _ = dk.dead_groups(dk.dead_ksteps(acts[h][:, :, torch.as_tensor(order[l]).long().cpu()]))
        out[h] = (n, lead)
    return out


@pytest.mark.parametrize("family", ["base", "white", "trained"])
def test_three_settings_are_bit_equal_on_real_weights(amd, oracle, family_sd, monkeypatch, family):
    """Every inference entry on the 64-ray scene of tests/test_gpu_dead_ksteps.py (64 coarse depths on the coarse model, 192 sorted
    depths on the fine one, and 37 explicit points), through packed_inference of a network calibrated on those rays and through
    the identity stream.  Before any launch the CPU activations under the calibrated order show what the inputs exercise."""
    sc = _scene(oracle, family_sd, family)
    monkeypatch.delenv("NERF_UNIT_ORDER", raising=False)
    net = network(amd, sc["sd"], "f32", train=False)
    ren = amd.Renderer(net)
    orders = ren.calibrate_unit_order({"rays_o": sc["o"][None].cuda(), "rays_d": sc["d"][None].cuda()})
    assert net.packed_inference("fine").data_ptr() != net.packed("fine").data_ptr()
    if family == "base":
        fine = _ordered_leading(sc["acts"]["fine"], orders["fine"])
        tiles = fine["h1"][1].numel()
        for h in ("h1", "h2", "h3", "h4", "h6", "h7"):
            assert (fine[h][1] > 0).sum().item() * 2 >= tiles, (h, "a prefix in fewer than half of the tiles")
        lead = torch.stack([fine[h][1] for h in RELU_FED])
        n_dead = torch.stack([fine[h][0] for h in RELU_FED])
        print("fine, ordered: mean leading run per layer", [round(x, 2) for x in lead.float().mean(1).tolist()])
        assert (lead == 0).any(), "no tile without a prefix"
        assert (n_dead > lead).any(), "no all-dead group outside a prefix"
        assert (lead % 2 == 1).any() and ((lead % 2 == 0) & (lead > 0)).any(), "both slot parities"
    o, d = sc["o"].cuda(), sc["d"].cuda()
    L = amd._lib
    for stream in (net.packed_inference, net.packed):
        for t, model in ((sc["t_c"], ""), (sc["t_f"], "fine")):
            t = t.cuda()
            n, S = t.shape
            for fn in RAY_ENTRIES:
                def rays():
                    raw = torch.full((n, S, 4), float("nan"), device="cuda")
                    L.call(fn, o, d, t, S, n, S, stream(model), raw, 0)
                    torch.cuda.synchronize()
                    return raw
                on, rows, off = _three(monkeypatch, rays)
                assert torch.isfinite(on).all() and on[..., 3].abs().max() > 0, (fn, model)
                assert torch.equal(_bits(on), _bits(rows)) and torch.equal(_bits(on), _bits(off)), (family, fn, model)
        pts = oracle.points_on_rays(sc["o"][:1], sc["d"][:1], sc["t_f"][:1])[0, :37].reshape(37, 1, 3).contiguous().cuda()
        vd = (sc["d"][:1] / sc["d"][:1].norm(dim=-1, keepdim=True)).expand(37, 3).contiguous().cuda()

        def points():
            raw = torch.full((37, 1, 4), float("nan"), device="cuda")
            L.call("nerf_mlp_forward", pts, vd, 37, 1, stream("fine"), raw, 0)
            torch.cuda.synchronize()
            return raw
        on, rows, off = _three(monkeypatch, points)
        assert torch.isfinite(on).all() and torch.equal(_bits(on), _bits(rows)) and torch.equal(_bits(on), _bits(off)), family
