"""Unit orders of the fp32 render MLP on the GPU (include/nerf_mi355x_order.h): the ordered pack against
nerf_pack_model of the host-permuted state dict, exact integer probes on every inference entry (the ordered stream is the same
network: where every sum is exact in any order, raw is bit-equal), the statistics kernel against a torch restatement, real weights
against the oracle inside the bounds of tests/test_gpu_parity.py, and the renderer's plumbing."""
import pytest
import torch

import f16_reference as F
import pack_reference as PR
import unit_order_reference as U
from gpu_common import amd, network  # noqa: F401
from test_gpu_parity import RAW_RTOL, _chan_err, assert_image_close

pytestmark = pytest.mark.gpu

PREFIX = {"": "model", "fine": "model_fine"}


def _bits(x):
    return x.contiguous().view(torch.int32)


def _sub(sd, model):
    p = PREFIX[model] + "."
    return {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}


def _pack(amd, net, model, order=None, entry="ordered", precision=0):
    """The stream of net's `model` through nerf_pack_model_ordered (order: [8,256] or None) or nerf_pack_model, as float32."""
    L = amd._lib
    params = [p.detach().contiguous() for p in (net.model_fine if model == "fine" else net.model).ordered_params()]
    out = torch.full((L.packed_model_bytes(precision),), 0xA5, dtype=torch.uint8, device="cuda")
    if entry == "ordered":
        dev_order = None if order is None else torch.as_tensor(order).to(device="cuda", dtype=torch.uint8).contiguous()
        L.call("nerf_pack_model_ordered", params, dev_order, out, precision)
    else:
        L.call("nerf_pack_model", params, out, precision)
    torch.cuda.synchronize()
    return out


def _ordered_net(amd, sd, orders):
    """A network with `sd` and the given {model: order} attached (packed_inference is then the ordered stream)."""
    net = network(amd, sd, "f32")
    for model, order in orders.items():
        net.set_unit_order(model, order)
    return net


# ------------------------------------------------------------------------------------------------ 1. ordered pack
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ordered_pack_equals_the_pack_of_the_permuted_state_dict(amd, family_sd, seed):
    """Byte for byte, the fold region included, for the coarse and the fine model under a seeded random order."""
    sd = family_sd("trained" if seed == 2 else "base")
    orders = {"": U.random_orders(10 + seed), "fine": U.random_orders(20 + seed)}
    net = network(amd, sd, "f32")
    perm = network(amd, U.permute_state_dict(sd, {PREFIX[m]: o for m, o in orders.items()}), "f32")
    for model in ("", "fine"):
        got = _pack(amd, net, model, orders[model])
        want = _pack(amd, perm, model, entry="plain")
        assert torch.equal(got, want), model
        assert not torch.equal(got, _pack(amd, net, model, entry="plain"))
        fold = slice(4 * PR.OFF_FOLD, 4 * (PR.OFF_FOLD + PR.FOLD_FLOATS))
        assert got.numel() == fold.stop and torch.equal(got[fold], want[fold])
        assert got[fold].view(torch.float32)[:PR.FOLD_OFF_DIR].abs().max() > 0


def test_null_table_is_nerf_pack_model_and_other_precisions_are_refused(amd, family_sd):
    net = network(amd, family_sd("base"), "f32")
    for model in ("", "fine"):
        assert torch.equal(_pack(amd, net, model, None), _pack(amd, net, model, entry="plain"))
    ident = torch.arange(256).expand(8, 256)
    assert torch.equal(_pack(amd, net, "fine", ident), _pack(amd, net, "fine", entry="plain"))
    L = amd._lib
    for name in ("f16", "f16m32", "f32x"):
        with pytest.raises(L.NerfLibraryError, match="f32 only"):
            _pack(amd, net, "fine", ident, precision=L.PRECISIONS[name])
    with pytest.raises(ValueError):
        net.set_unit_order("fine", torch.zeros(8, 256))


# ------------------------------------------------------------------------------------------------ 2. exact integer probes
POINT_COUNTS = ((1, 1), (1, 31), (3, 11), (5, 13))                # (rays, samples): 1, 31, 33 and 65 points


def _probe_nets(amd, seed, zero_axis):
    """(identity network, [networks under two random orders]) of one probe network, coarse = fine."""
    sd = F.both_models(F.probe_network(seed, zero_axis))
    sd = {k: v.contiguous() for k, v in sd.items()}
    ordered = [_ordered_net(amd, sd, {"": U.random_orders(100 * seed + k), "fine": U.random_orders(100 * seed + 50 + k)}) for k in (0, 1)]
    return network(amd, sd, "f32"), ordered, sd


@pytest.mark.parametrize("seed,zero_axis", [(0, 0), (1, 1), (2, 2)])
def test_integer_probes_are_bit_equal_on_every_inference_entry(amd, seed, zero_axis):
    """Probe networks of tests/f16_reference.py: +-1 weights, integer biases, points on the 1/4 grid with sin = 0 / cos = 1 on the
    encodings' live columns, so every sum is a multiple of 1/4 far below 2^24 and exact in any order (shown first: the identity
    stream equals the float64 oracle exactly).  Then raw of the ordered streams is int32-equal to the identity stream's on rays,
    density-only, for-compositing (with dead tiles), the masked list and points."""
    L = amd._lib
    ident, ordered, sd = _probe_nets(amd, seed, zero_axis)
    gen = torch.Generator().manual_seed(5000 + seed)

    def rays_raw(net, fn, o, d, t, n, S):
        raw = torch.full((n, S, 4), float("nan"), device="cuda")
        L.call(fn, o, d, t, S, n, S, net.packed_inference("fine"), raw, 0)
        torch.cuda.synchronize()
        return raw

    dead_seen = live_seen = False
    for n, S in POINT_COUNTS + ((6, 32), (4, 64)):
        o, d, t, pts, unit = F.probe_rays(gen, zero_axis, 256 if S == 32 else n, S, per_ray=True)
        if S == 32:                        # one tile per ray: three rays without a single sigma > 0 and three with, out of 256 candidates
            sig = F.probe_forward(_sub(sd, "fine"), pts.reshape(-1, 3), unit[:, None, :].expand(256, S, 3).reshape(-1, 3))[:, 3]
            live = (sig.reshape(256, S) > 0).any(-1)
            pick = torch.cat([(~live).nonzero()[:3, 0], live.nonzero()[:3, 0]])
            assert len(pick) == n, "the candidates hold too few dead or live tiles"
            o, d, t, pts, unit = (x[pick].contiguous() for x in (o, d, t, pts, unit))
        oc, dc, tc = o.cuda(), d.cuda(), t.cuda().contiguous()
        want = F.probe_forward(_sub(sd, "fine"), pts.reshape(-1, 3), unit[:, None, :].expand(n, S, 3).reshape(-1, 3)).reshape(n, S, 4)
        for fn in ("nerf_mlp_forward_rays", "nerf_mlp_forward_rays_density", "nerf_mlp_forward_rays_for_compositing"):
            base = rays_raw(ident, fn, oc, dc, tc, n, S)
            assert torch.isfinite(base).all()
            assert torch.equal(base[..., 3].cpu(), want[..., 3]), (fn, n, S)                  # exact: the premise of the probe
            if fn == "nerf_mlp_forward_rays":
                assert torch.equal(base.cpu(), want), (n, S)
            if fn == "nerf_mlp_forward_rays_for_compositing" and (n * S) % 32 == 0:
                tiles = (base[..., 3].reshape(-1, 32) > 0).any(-1)
                dead_seen, live_seen = dead_seen or bool((~tiles).any()), live_seen or bool(tiles.any())
            for net in ordered:
                assert torch.equal(_bits(rays_raw(net, fn, oc, dc, tc, n, S)), _bits(base)), (fn, n, S)
        # points: the same points, one direction each
        P = n * S
        p3, v3 = pts.reshape(P, 1, 3).contiguous().cuda(), unit[:, None, :].expand(n, S, 3).reshape(P, 3).contiguous().cuda()

        def points_raw(net):
            raw = torch.full((P, 1, 4), float("nan"), device="cuda")
            L.call("nerf_mlp_forward", p3, v3, P, 1, net.packed_inference("fine"), raw, 0)
            torch.cuda.synchronize()
            return raw
        base = points_raw(ident)
        assert torch.equal(base.reshape(n, S, 4).cpu(), want)
        for net in ordered:
            assert torch.equal(_bits(points_raw(net)), _bits(base)), (n, S)
    assert dead_seen and live_seen, "the for-compositing cases must hold a tile without density and one with"


@pytest.mark.parametrize("seed,zero_axis", [(0, 0), (1, 2)])
def test_integer_probes_masked_list(amd, seed, zero_axis):
    """An inference launch on a compacted index list: the coarse-only frame with a culling bitfield (seeded random words over a
    16^3-cell box) evaluates the kept samples by id and leaves the others zero.  The 64 depths are on the 1/16 grid and the
    directions are unit axis vectors, so the points stay exact; the fine pass is left out because its sampled depths are not.
    rgb, depth and the number of evaluated samples are int32-equal between the identity and the ordered streams, for 1, 31, 33 and
    65 rays, with ragged lists among them."""
    L = amd._lib
    ident, ordered, _ = _probe_nets(amd, seed, zero_axis)
    gen = torch.Generator().manual_seed(6000 + seed)
    o_all, _, _, _, unit = F.probe_rays(gen, zero_axis, 65, 1, per_ray=False)
    o_all, d_all = (o_all - 2.0 * unit).contiguous(), unit.contiguous()       # o + d t, t in [2, 6): |coordinates| < 8
    t_c = (2.0 + torch.arange(64, dtype=torch.float32) / 16).cuda()
    u = torch.linspace(0.0, 1.0, 128).cuda()
    words = int(L.call("nerf_occupancy_words", 17, 17, 17))
    bits = torch.randint(-2 ** 31, 2 ** 31, (words,), generator=gen, dtype=torch.int64).to(torch.int32).cuda()

    def frame(net, n):
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
        base = frame(ident, n)
        assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all() and 0 < base[2] < 64 * n, (n, base[2])
        ragged = ragged or base[2] % 32 != 0
        for net in ordered:
            got = frame(net, n)
            assert got[2] == base[2], n
            assert torch.equal(_bits(got[0]), _bits(base[0])) and torch.equal(_bits(got[1]), _bits(base[1])), n
    assert ragged


# ------------------------------------------------------------------------------------------------ 3. statistics kernel
def _save_layout(P):
    pad = (P + 31) // 32 * 32
    return pad, [pad * (96 + 256 * l) for l in range(8)]


@pytest.mark.parametrize("shape", ["4x192", "ragged77"])
def test_statistics_kernel_equals_the_torch_restatement(amd, oracle, family_sd, shape):
    """Counts, so exactly: 4 rays x 192 samples through the ray-mode SAVE forward (24 tiles), and 77 explicit points (two tiles and
    a ragged third, whose idle lanes repeat point 76).  The restatement reads the saved h rows of the same buffer."""
    L = amd._lib
    net = network(amd, family_sd("base"), "f32")
    ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(9))[:4]
    o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(40.0), pixel_ids=ids)
    if shape == "4x192":
        P, t = 4 * 192, torch.linspace(2.0, 6.0, 192).cuda()
        save = torch.zeros(int(L.call("nerf_train_save_floats", P)), device="cuda")
        raw = torch.empty(4, 192, 4, device="cuda")
        L.call("nerf_mlp_forward_rays_save", o.cuda(), d.cuda(), t, 0, 4, 192, net.packed("fine"), raw, save, 0)
    else:
        P = 77
        t = torch.linspace(2.0, 6.0, 77)
        pts = (o[:1] + d[:1] * t[:, None]).reshape(P, 1, 3).contiguous().cuda()
        vd = (d[:1] / d[:1].norm(dim=-1, keepdim=True)).expand(P, 3).contiguous().cuda()
        save = torch.zeros(int(L.call("nerf_train_save_floats", P)), device="cuda")
        raw = torch.empty(P, 1, 4, device="cuda")
        L.call("nerf_mlp_forward_points_save", pts, vd, P, 1, net.packed("fine"), raw, save, 0)
    counts = torch.full((8, 256, 256), -1, dtype=torch.int32, device="cuda")
    L.call("nerf_unit_order_stats", save, P, counts)
    torch.cuda.synchronize()
    pad, offs = _save_layout(P)
    for l in range(8):
        h = save[offs[l]:offs[l] + pad * 256].reshape(pad, 256)[:P].cpu()
        h = torch.cat([h, h[-1:].expand(pad - P, 256)])                      # a ragged tile counts with the points it has
        want = U.co_dead_counts(h.reshape(pad // 32, 32, 256))
        assert torch.equal(counts[l].cpu(), want), l
        assert 0 < int(want.diagonal().max()) <= pad // 32 and int(want.max()) == int(want.diagonal().max())
    assert L.load().nerf_unit_order_stats(None, 32, counts.data_ptr(), None) != 0
    assert L.load().nerf_unit_order_stats(save.data_ptr(), 0, counts.data_ptr(), None) != 0


# ------------------------------------------------------------------------------------------------ 4. real weights
_REAL = {}


def _real_scene(oracle, family_sd, family):
    """64 seeded rays of the bench frame and the oracle's render of them, once per family."""
    if family not in _REAL:
        sd = family_sd(family)
        ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(0))[:64]
        o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(40.0), pixel_ids=ids)
        with torch.no_grad():
            rgb, dep, parts = oracle.render(sd, o[None], d[None], return_parts=True)
            pts = oracle.points_on_rays(o, d, parts["t_sorted"])
            raw = oracle.network_forward(sd, pts, parts["viewdirs"], "fine")
        _REAL[family] = dict(sd=sd, o=o.contiguous(), d=d.contiguous(), rgb=rgb, dep=dep, pts=pts, vd=parts["viewdirs"], raw=raw)
    return _REAL[family]


@pytest.mark.parametrize("kind", ["calibrated", "random"])
@pytest.mark.parametrize("family", ["base", "trained"])
def test_real_weights_stay_inside_the_fp32_bounds(amd, oracle, family_sd, family, kind):
    """raw on the oracle's 64 x 192 fine points within RAW_RTOL per channel, rendered rgb and depth of the 64 rays within
    assert_image_close's family bounds: the figures tests/test_gpu_parity.py holds the identity stream to."""
    sc = _real_scene(oracle, family_sd, family)
    net = network(amd, sc["sd"], "f32")
    ren = amd.Renderer(net)
    batch = {"rays_o": sc["o"][None].cuda(), "rays_d": sc["d"][None].cuda()}
    ident_raw = net.forward(sc["pts"].cuda(), sc["vd"].cuda(), None, model="fine")
    if kind == "calibrated":
        orders = ren.calibrate_unit_order(batch)
        assert set(orders) == {"", "fine"} and all(o.shape == (8, 256) for o in orders.values())
    else:
        net.set_unit_order("", U.random_orders(31))
        net.set_unit_order("fine", U.random_orders(32))
    assert net.packed_inference("fine").data_ptr() != net.packed("fine").data_ptr()
    L = amd._lib
    P = 64 * 192
    raw = torch.empty(P, 1, 4, device="cuda")
    vd = sc["vd"][:, None, :].expand(64, 192, 3).reshape(P, 3).contiguous().cuda()
    L.call("nerf_mlp_forward", sc["pts"].reshape(P, 1, 3).contiguous().cuda(), vd, P, 1, net.packed_inference("fine"), raw, 0)
    raw = raw.reshape(64, 192, 4)
    err = _chan_err(raw, sc["raw"])
    print(family, kind, "raw error", err, "identity", _chan_err(ident_raw, sc["raw"]))
    assert err <= RAW_RTOL
    assert not torch.equal(_bits(raw), _bits(ident_raw))                     # (the ordered stream is really another summation order)
    with torch.no_grad():
        rgb, dep = ren.render(batch)
    assert_image_close(oracle, rgb, dep, sc["rgb"], sc["dep"], family=family)


# ------------------------------------------------------------------------------------------------ 5. plumbing
def _batch(sc, n):
    return {"rays_o": sc["o"][None, :n].cuda(), "rays_d": sc["d"][None, :n].cuda()}


def test_auto_calibration_threshold_capture_and_switch(amd, oracle, family_sd, monkeypatch):
    sc = _real_scene(oracle, family_sd, "base")
    monkeypatch.delenv("NERF_UNIT_ORDER", raising=False)
    with torch.no_grad():
        plain = amd.Renderer(network(amd, sc["sd"], "f32")).render(_batch(sc, 64))        # (default threshold: never calibrates)
        # below the threshold: never
        net = network(amd, sc["sd"], "f32")
        ren = amd.Renderer(net)
        ren.unit_order_min_rays = 64
        for _ in range(3):
            small = ren.render(_batch(sc, 63))
        assert net.unit_order("") is None and net.unit_order("fine") is None
        assert torch.equal(small[0], plain[0][:63]) and torch.equal(small[1], plain[1][:63])
        # at the threshold: the first call only announces the weights, the second calibrates
        first = ren.render(_batch(sc, 64))
        assert net.unit_order("fine") is None and torch.equal(first[0], plain[0]) and torch.equal(first[1], plain[1])
        second = ren.render(_batch(sc, 64))
        assert net.unit_order("") is not None and net.unit_order("fine") is not None
        assert sorted(net.unit_order("fine")[3].tolist()) == list(range(256))
        assert (second[0] - plain[0]).abs().max() <= 1e-5 and not (torch.equal(second[0], plain[0]) and torch.equal(second[1], plain[1]))
        # an order, once there, serves calls of any size: a subset rendered alone stays bit-identical
        sub = ren.render(_batch(sc, 33))
        assert torch.equal(sub[0], second[0][:33]) and torch.equal(sub[1], second[1][:33])
        # "off" and NERF_UNIT_ORDER=0: the identity stream, bit for bit
        off = amd.Renderer(net)
        off.unit_order = "off"
        got = off.render(_batch(sc, 64))
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
        monkeypatch.setenv("NERF_UNIT_ORDER", "0")
        got = ren.render(_batch(sc, 64))
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
        monkeypatch.delenv("NERF_UNIT_ORDER")
        # render_geometry reads the streams render() reads
        geo = ren.render_geometry(_batch(sc, 64))
        assert torch.equal(geo["rgb"], second[0]) and torch.equal(geo["depth"], second[1])
        assert torch.isfinite(geo["normal"]).all() and torch.isfinite(geo["acc"]).all()
        # an in-place weight update invalidates the fine order, and the next two large calls calibrate again
        net.model_fine.pts_linears[2].bias.add_(0.0)
        assert net.unit_order("fine") is None and net.unit_order("") is not None
        assert net.packed_inference("fine").data_ptr() == net.packed("fine").data_ptr()
        ren.render(_batch(sc, 64))
        assert net.unit_order("fine") is None
        ren.render(_batch(sc, 64))
        assert net.unit_order("fine") is not None


def test_no_calibration_during_graph_capture(amd, oracle, family_sd, monkeypatch):
    sc = _real_scene(oracle, family_sd, "base")
    monkeypatch.delenv("NERF_UNIT_ORDER", raising=False)
    net = network(amd, sc["sd"], "f32")
    ren = amd.Renderer(net)
    ren.unit_order_min_rays = 64
    b = _batch(sc, 64)
    with torch.no_grad():
        eager = ren.render(b)                                                # the first large call: announces, packs, builds tables
        torch.cuda.synchronize()
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                g_rgb, g_dep = ren.render(b)                                 # would be the calibrating call: a capture uses what exists
        torch.cuda.current_stream().wait_stream(side)
        assert net.unit_order("") is None and net.unit_order("fine") is None
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_rgb, eager[0]) and torch.equal(g_dep, eager[1])
        ren.render(b)
        assert net.unit_order("fine") is not None
