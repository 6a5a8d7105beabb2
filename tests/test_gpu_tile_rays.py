"""Tile shape of the fp32 inference ray instances (csrc/nerf_mlp_f32.hip.inc prologue, MlpArgs::tile_rays_log2, DESIGN.md section
2.1 "Tile shape"): under NERF_TILE_RAYS=R a 32-point tile is R neighbouring rays by 32 / R consecutive samples instead of 32
consecutive samples of one ray.  The shape decides which k-steps are dead tile-wide and which tiles skip the colour branch; it
never enters a value.  So every comparison here is int32-equal: `raw` per entry, the dead-colour rule on the tiles of the shape,
composited rgb and depth, whole frames, and everything the switch must not touch (listed passes, the training kernels)."""
import pytest
import torch

from gpu_common import amd, assert_grads_equal, network  # noqa: F401
from wgrad_reference import PARAM_SHAPES

pytestmark = pytest.mark.gpu

SWITCH = "NERF_TILE_RAYS"
SHAPES = (2, 4, 8, 32)
FAMILIES = ("base", "white", "trained")
N = 37                      # rays of the scene: ragged for every shape
PIXEL = 300 * 800 + 400     # the run starts here (row 300 of the bench frame): the silhouette of all three families crosses it
SENTINEL = -7.25
PAD = 4096                  # floats in front of and behind `raw`


def _bits(x):
    return x.contiguous().view(torch.int32)


def _with(monkeypatch, value, run):
    """run() with NERF_TILE_RAYS = value (None: unset)."""
    monkeypatch.delenv(SWITCH, raising=False)
    if value is not None:
        monkeypatch.setenv(SWITCH, str(value))
    try:
        return run()
    finally:
        monkeypatch.delenv(SWITCH, raising=False)


def tile_live(sig, R):
    """sig [n, S] -> bool [n, S]: the tile of R rays by 32 / R samples that holds the point has a sigma > 0.  Rays past n (a ragged
    last group) add nothing: the kernel's padding lanes repeat a point of the tile and take no part in the ballot."""
    n, S = sig.shape
    s = 32 // R
    assert S % s == 0
    G = (n + R - 1) // R
    pos = torch.zeros(G * R, S, dtype=torch.bool, device=sig.device)
    pos[:n] = sig > 0
    live = pos.reshape(G, R, S // s, s).any(3).any(1)
    return live[:, None, :, None].expand(G, R, S // s, s).reshape(G * R, S)[:n]


_SCENES = {}


def _scene(oracle, family_sd, family):
    """37 consecutive pixels of one row of the bench frame: rays, the shared coarse table, the oracle's 192 sorted depths per ray
    and its fine sigma (CPU).  Computed once per family, never modified."""
    if family not in _SCENES:
        sd = family_sd(family)
        o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(40.0), pixel_ids=torch.arange(PIXEL, PIXEL + N))
        with torch.no_grad():
            _, _, parts = oracle.render(sd, o[None], d[None], return_parts=True)
        _SCENES[family] = dict(sd=sd, o=o.contiguous(), d=d.contiguous(), t_c=parts["t_coarse"][0].contiguous(),
                               t_f=parts["t_sorted"].contiguous(), sigma_f=parts["raw_fine"][..., 3].contiguous())
    return _SCENES[family]


def _forward(amd, fn, packed, o, d, t, stride, n, S):
    """One ray entry on the first n rays; `raw` sits inside a sentinel-filled buffer -> (raw [n, S, 4], sentinels intact)."""
    buf = torch.full((2 * PAD + n * S * 4,), SENTINEL, device="cuda")
    raw = buf[PAD:PAD + n * S * 4]
    raw.fill_(float("nan"))
    amd._lib.call(fn, o[:n].contiguous(), d[:n].contiguous(), t if stride == 0 else t[:n].contiguous(), stride, n, S, packed, raw, 0)
    torch.cuda.synchronize()
    intact = bool((buf[:PAD] == SENTINEL).all() and (buf[PAD + n * S * 4:] == SENTINEL).all())
    return raw.view(n, S, 4).clone(), intact


def _t_tables(sc):
    """(t, stride, S): 64 and 192 samples, each once as a shared table (stride 0) and once per ray."""
    t_c, t_f = sc["t_c"].cuda(), sc["t_f"].cuda()
    return ((t_c, 0, 64), (t_f[:, ::3].contiguous(), 64, 64), (t_f[0].contiguous(), 0, 192), (t_f, 192, 192))


# ------------------------------------------------------------------------------------------------ non-vacuity (CPU oracle)
@pytest.mark.parametrize("family", FAMILIES)
def test_scene_exercises_the_shapes(oracle, family_sd, family):
    """With the oracle's fine sigma every shape has a dead tile, a live tile, and points whose tile is dead under one of R and 1
    and live under the other: the dead-colour tests below compare different decisions, not the same one twice."""
    sig = _scene(oracle, family_sd, family)["sigma_f"]
    one = tile_live(sig, 1)
    for R in SHAPES:
        shaped = tile_live(sig, R)
        assert (~shaped).any() and shaped.any() and (shaped != one).any(), (family, R)


# ------------------------------------------------------------------------------------------------ raw per entry
@pytest.mark.parametrize("family", FAMILIES)
def test_raw_is_bit_equal_per_entry(amd, oracle, family_sd, monkeypatch, family):
    """The density entry and nerf_mlp_forward_rays, 64 and 192 samples, shared and per-ray t, n_rays in {1, R - 1, R, R + 1, 37}:
    `raw` of every valid ray is written and int32-equal to one-ray tiles, and nothing outside `raw` is touched."""
    sc = _scene(oracle, family_sd, family)
    net = network(amd, sc["sd"], "f32", train=False)
    o, d = sc["o"].cuda(), sc["d"].cuda()
    for fn, model in (("nerf_mlp_forward_rays_density", ""), ("nerf_mlp_forward_rays", "fine")):
        for t, stride, S in _t_tables(sc):
            ref = {}
            for R in SHAPES:
                for n in sorted({1, R - 1, R, R + 1, N} - {0}):
                    if n not in ref:
                        ref[n], ok = _with(monkeypatch, 1, lambda: _forward(amd, fn, net.packed(model), o, d, t, stride, n, S))
                        assert ok and torch.isfinite(ref[n]).all() and ref[n][..., 3].abs().max() > 0
                    got, ok = _with(monkeypatch, R, lambda: _forward(amd, fn, net.packed(model), o, d, t, stride, n, S))
                    assert ok, ("sentinel overwritten", fn, S, stride, R, n)
                    assert torch.isfinite(got).all(), ("a row of a valid ray was not written", fn, S, stride, R, n)
                    assert torch.equal(_bits(got), _bits(ref[n])), (family, fn, S, stride, R, n)


# ------------------------------------------------------------------------------------------------ dead-colour rule on shaped tiles
@pytest.mark.parametrize("family", FAMILIES)
def test_dead_colour_rule_follows_the_shape(amd, oracle, family_sd, monkeypatch, family):
    """nerf_mlp_forward_rays_for_compositing on the 37 rays x 192 sorted depths: sigma is int32-equal to one-ray tiles; a colour is
    the full network's, bit for bit, or exactly 0, and 0 exactly where the point's R-shaped tile (cut from sigma itself) has no
    sigma > 0; nerf_composite gives int32-equal rgb and depth."""
    sc = _scene(oracle, family_sd, family)
    net = network(amd, sc["sd"], "f32", train=False)
    o, d, t = sc["o"].cuda(), sc["d"].cuda(), sc["t_f"].cuda()
    pk = net.packed("fine")
    full, ok = _with(monkeypatch, 1, lambda: _forward(amd, "nerf_mlp_forward_rays", pk, o, d, t, 192, N, 192))
    assert ok

    def composite(raw):
        rgb, dep = torch.full((N, 3), float("nan"), device="cuda"), torch.full((N,), float("nan"), device="cuda")
        amd._lib.call("nerf_composite", raw.contiguous(), t, 192, N, 192, 1, rgb, dep, None)
        torch.cuda.synchronize()
        return rgb, dep

    outs = {}
    for R in (1,) + SHAPES:
        raw, ok = _with(monkeypatch, R, lambda: _forward(amd, "nerf_mlp_forward_rays_for_compositing", pk, o, d, t, 192, N, 192))
        assert ok
        assert torch.equal(_bits(raw[..., 3]), _bits(full[..., 3])), (family, R)
        live = tile_live(raw[..., 3], R)
        assert torch.equal(_bits(raw[..., :3][live]), _bits(full[..., :3][live])), (family, R)
        assert torch.all(_bits(raw[..., :3][~live]) == 0), (family, R)
        outs[R] = (live, *composite(raw))
        assert torch.isfinite(outs[R][1]).all() and torch.isfinite(outs[R][2]).all()
    for R in SHAPES:
        assert (~outs[R][0]).any() and outs[R][0].any() and (outs[R][0] != outs[1][0]).any(), (family, R, "vacuous on the GPU's sigma")
        assert torch.equal(_bits(outs[R][1]), _bits(outs[1][1])) and torch.equal(_bits(outs[R][2]), _bits(outs[1][2])), (family, R)


# ------------------------------------------------------------------------------------------------ whole frames
def _frame_scene(oracle, family_sd):
    """70 consecutive pixels of the same row: with NERF_RENDER_BLOCK_RAYS=64 two blocks, the second (6 rays) ragged for every R."""
    sd = family_sd("base")
    o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(40.0), pixel_ids=torch.arange(PIXEL - 16, PIXEL + 54))
    return sd, o.contiguous().cuda(), d.contiguous().cuda()


def _render(amd, ren, packed, o, d, fast_sampling=0, draws=None):
    L = amd._lib
    n = o.shape[0]
    t_c, u = ren._get_tables(torch.device("cuda", torch.cuda.current_device()))
    rgb, dep = torch.full((n, 3), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
    if draws is None:
        ws = torch.empty(int(L.call("nerf_render_workspace_bytes", n, 128, fast_sampling)), dtype=torch.uint8, device="cuda")
        L.call("nerf_render_forward", o, d, n, packed(""), packed("fine"), t_c, u, 128, 1, 0, fast_sampling, 0.25, ws, ws.numel(), rgb, dep)
    else:
        ws = torch.empty(int(L.call("nerf_render_stochastic_workspace_bytes", n, 128)), dtype=torch.uint8, device="cuda")
        L.call("nerf_render_forward_stochastic", o, d, n, packed(""), packed("fine"), t_c, u, draws[0], draws[1], 128, 1, 0, 0, 0.25,
               ws, ws.numel(), rgb, dep)
    torch.cuda.synchronize()
    assert torch.isfinite(rgb).all() and torch.isfinite(dep).all()
    return rgb, dep


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize("ordered", [False, True])
def test_whole_frames_are_bit_equal(amd, oracle, family_sd, monkeypatch, ordered):
    """nerf_render_forward and nerf_render_forward_stochastic on 70 rays in two blocks: rgb and depth under NERF_TILE_RAYS = 2, 4, 8
    and unset (the shipped default) are int32-equal to NERF_TILE_RAYS=1, with and without an installed unit order, and with
    NERF_DEAD_KSTEP_SKIP=0 as well."""
    sd, o, d = _frame_scene(oracle, family_sd)
    monkeypatch.setenv("NERF_RENDER_BLOCK_RAYS", "64")
    monkeypatch.delenv("NERF_UNIT_ORDER", raising=False)
    net = network(amd, sd, "f32", train=False)
    ren = amd.Renderer(net)
    packed = net.packed
    if ordered:
        ren.calibrate_unit_order({"rays_o": o[None], "rays_d": d[None]})
        packed = net.packed_inference
        assert packed("fine").data_ptr() != net.packed("fine").data_ptr()
    gen = torch.Generator().manual_seed(11)
    draws = (torch.rand(70, 64, generator=gen).cuda(), torch.rand(70, 128, generator=gen).cuda())
    for skip in (None, "0"):
        monkeypatch.delenv("NERF_DEAD_KSTEP_SKIP", raising=False)
        if skip is not None:
            monkeypatch.setenv("NERF_DEAD_KSTEP_SKIP", skip)
        for dr in (None, draws):
            one = _with(monkeypatch, 1, lambda: _render(amd, ren, packed, o, d, draws=dr))
            for R in (2, 4, 8, None):
                got = _with(monkeypatch, R, lambda: _render(amd, ren, packed, o, d, draws=dr))
                assert _same(got, one), (ordered, skip, dr is not None, R)
    monkeypatch.delenv("NERF_DEAD_KSTEP_SKIP", raising=False)


def test_listed_passes_do_not_hear_the_switch(amd, oracle, family_sd, monkeypatch):
    """A fast_sampling frame and an occupancy frame (both passes on lists): int32-equal with NERF_TILE_RAYS=1 (nothing shaped
    anywhere), unset and 4.  In the fast_sampling frame the dense coarse launch is shaped and its listed fine launch is not; in
    the occupancy frame both launches are listed."""
    sd, o, d = _frame_scene(oracle, family_sd)
    monkeypatch.setenv("NERF_RENDER_BLOCK_RAYS", "64")
    net = network(amd, sd, "f32", train=False)
    ren = amd.Renderer(net)
    L = amd._lib
    n = o.shape[0]
    t_c, u = ren._get_tables(torch.device("cuda", torch.cuda.current_device()))
    words = int(L.call("nerf_occupancy_words", 17, 17, 17))
    bits = torch.randint(-2 ** 31, 2 ** 31, (words,), generator=torch.Generator().manual_seed(5), dtype=torch.int64).to(torch.int32).cuda()

    def occupancy():
        ws = torch.empty(int(L.call("nerf_render_occupancy_workspace_bytes", n, 128, 0)), dtype=torch.uint8, device="cuda")
        rgb, dep = torch.full((n, 3), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        evaluated = torch.zeros(2, dtype=torch.int64, device="cuda")
        L.call("nerf_render_forward_occupancy", o, d, n, net.packed(""), net.packed("fine"), t_c, u, 128, 1, 0, 0, 0.25,
               bits, bits, [17, 17, 17], [-8.0, -8.0, -8.0], [1.0, 1.0, 1.0], evaluated, ws, ws.numel(), rgb, dep)
        torch.cuda.synchronize()
        ev = evaluated.tolist()
        assert 0 < ev[0] < 64 * n and 0 < ev[1] < 192 * n, ev               # both passes ran on lists
        return rgb, dep
    for run in (lambda: _render(amd, ren, net.packed, o, d, fast_sampling=1), occupancy):
        one = _with(monkeypatch, 1, run)
        assert torch.isfinite(one[0]).all() and torch.isfinite(one[1]).all()
        for R in (None, 4):
            assert _same(_with(monkeypatch, R, run), one), R


# ------------------------------------------------------------------------------------------------ training is deaf to the switch
def test_training_kernels_do_not_hear_the_switch(amd, oracle, family_sd, monkeypatch):
    """With NERF_TILE_RAYS=4 the SAVE forward's `raw` and save buffer and one backward's per-point outputs (the gradient rows of
    every layer and g_t) are int32-equal to the run without it.  The parameter gradients are sums of those rows that the
    weight-gradient kernels add up with float atomics, in an order that changes from call to call
    (on the MI355X dW of layer 0 differed in its last bits between two calls whose per-point rows were int32-equal); they read nothing but rows shown equal
    above and never see MlpArgs, and are held to the project's form and bound for regrouped atomic sums of identical terms
    (gpu_common.assert_grads_equal: 1e-4 of the tensor's maximum, exact zeros kept)."""
    sc = _scene(oracle, family_sd, "base")
    net = network(amd, sc["sd"], "f32", train=True)
    L = amd._lib
    n, S = 2, 64
    P = n * S
    o, d, t = sc["o"][:n].cuda().contiguous(), sc["d"][:n].cuda().contiguous(), sc["t_f"][:n, ::3].cuda().contiguous()
    draw = torch.randn(P, 4, generator=torch.Generator().manual_seed(2)).cuda()

    def step():
        save = torch.zeros(int(L.call("nerf_train_save_floats", P)), device="cuda")
        raw = torch.full((n, S, 4), float("nan"), device="cuda")
        L.call("nerf_mlp_forward_rays_save", o, d, t, S, n, S, net.packed("fine"), raw, save, 0)
        gsave = torch.zeros(int(L.call("nerf_train_grad_floats", P)), device="cuda")
        g_t = torch.zeros(P, device="cuda")
        grads = [torch.zeros(s, device="cuda") for s in PARAM_SHAPES]
        L.call("nerf_mlp_backward", o, d, t, S, n, S, net.packed_bwd("fine"), draw, save, gsave, g_t, grads, 0)
        torch.cuda.synchronize()
        return [raw, save, gsave, g_t] + grads
    off = _with(monkeypatch, None, step)
    on = _with(monkeypatch, 4, step)
    assert torch.isfinite(off[0]).all() and off[3].abs().max() > 0 and all(g.abs().max() > 0 for g in off[4:])
    for i, (a, b) in enumerate(zip(on[:4], off[:4])):
        assert torch.equal(_bits(a), _bits(b)), i
    assert_grads_equal(on[4:], off[4:])


# ------------------------------------------------------------------------------------------------ other values
def test_other_values_behave_as_unset(amd, oracle, family_sd, monkeypatch):
    """3, 0, 64 and abc are ignored: the direct entry keeps one-ray tiles and the frame its default.  Seen through the dead-colour
    decision, which follows the shape (the scene's tiles differ between every two shapes), and through a frame; 16 and 32 work at
    both sample counts."""
    sc = _scene(oracle, family_sd, "base")
    net = network(amd, sc["sd"], "f32", train=False)
    o, d, t = sc["o"].cuda(), sc["d"].cuda(), sc["t_f"].cuda()
    run = lambda: _forward(amd, "nerf_mlp_forward_rays_for_compositing", net.packed("fine"), o, d, t, 192, N, 192)[0]
    unset, one, four = _with(monkeypatch, None, run), _with(monkeypatch, 1, run), _with(monkeypatch, 4, run)
    assert torch.equal(_bits(unset), _bits(one)) and not torch.equal(_bits(four), _bits(one))
    for bad in ("3", "0", "64", "abc", "", "4x", "-4"):
        assert torch.equal(_bits(_with(monkeypatch, bad, run)), _bits(unset)), bad
    for R in (16, 32):
        raw = _with(monkeypatch, R, run)
        live = tile_live(raw[..., 3], R)
        assert torch.equal(_bits(raw[..., 3]), _bits(one[..., 3])) and torch.all(_bits(raw[..., :3][~live]) == 0) and (~live).any()
        for tt, stride, S in _t_tables(sc):
            for fn, model in (("nerf_mlp_forward_rays_density", ""), ("nerf_mlp_forward_rays", "fine")):
                ref, _ = _with(monkeypatch, 1, lambda: _forward(amd, fn, net.packed(model), o, d, tt, stride, N, S))
                got, ok = _with(monkeypatch, R, lambda: _forward(amd, fn, net.packed(model), o, d, tt, stride, N, S))
                assert ok and torch.equal(_bits(got), _bits(ref)), (R, S, stride, fn)
    # a sample count that 32 / R does not divide keeps one-ray tiles: 8 samples per ray and R = 2 (16 samples of a ray per tile)
    t8 = t[:, :8].contiguous()
    ref, _ = _with(monkeypatch, 1, lambda: _forward(amd, "nerf_mlp_forward_rays_for_compositing", net.packed("fine"), o, d, t8, 8, N, 8))
    got, ok = _with(monkeypatch, 2, lambda: _forward(amd, "nerf_mlp_forward_rays_for_compositing", net.packed("fine"), o, d, t8, 8, N, 8))
    assert ok and torch.equal(_bits(got), _bits(ref))
    # the frame: an ignored value is the default, which is bit-equal to every shape anyway; it must simply render
    sd, fo, fd = _frame_scene(oracle, family_sd)
    ren = amd.Renderer(net)
    one = _with(monkeypatch, 1, lambda: _render(amd, ren, net.packed, fo, fd))
    assert _same(_with(monkeypatch, "abc", lambda: _render(amd, ren, net.packed, fo, fd)), one)
