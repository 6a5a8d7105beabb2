"""tools/dead_ksteps.py --tile-rays: the probe cuts tiles of R neighbouring rays by 32 / R consecutive samples, as the fp32 inference
kernel does under NERF_TILE_RAYS=R ("Tile shape").  R = 1 is the tool as it was, the regrouping only
permutes points, and on the "base" family the shaped tiles leave fewer MFMAs in both launches."""
import contextlib
import io
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import dead_ksteps as dk  # noqa: E402

SHAPES = (1, 2, 4, 8, 16, 32)


def test_one_ray_tiles_are_the_tool_as_it_was(oracle, synthetic_sd):
    """R = 1: the pixels are the seeded scattered ones, the cut is 32 consecutive samples of a ray, and the figures equal those of
    the cut restated here (the tool's code before the shape existed)."""
    ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(3))[:24]
    assert torch.equal(dk.pixel_runs(24, 3, 1), ids)
    x = torch.arange(24 * 64 * 2, dtype=torch.float32).reshape(24 * 64, 2)
    assert torch.equal(dk.regroup(x, 24, 64, 1), x.reshape(24 * 64 // 32, 32, 2))
    got = dk.probe(synthetic_sd, n_rays=24, seed=3, calibrate_rays=16)
    assert got == dk.probe(synthetic_sd, n_rays=24, seed=3, calibrate_rays=16, tile_rays=1)
    # restated: scattered rays, plain reshape, calibration on seed + 1
    o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(40.0), pixel_ids=ids)
    with torch.no_grad():
        _, _, parts = oracle.render(synthetic_sd, o[None], d[None], return_parts=True)
    cal = dk.launch_tiles(synthetic_sd, 16, 4)
    for key, prefix, t in (("coarse", "model", parts["t_coarse"]), ("fine", "model_fine", parts["t_sorted"])):
        pts = oracle.points_on_rays(o, d, t)
        emb = torch.cat([oracle.freq_encode(pts.reshape(-1, 3), oracle.XYZ_FREQS),
                         oracle.freq_encode(parts["viewdirs"][:, None].expand(*pts.shape).reshape(-1, 3), oracle.DIR_FREQS)], -1)
        with torch.no_grad():
            raw, acts = oracle.nerf_mlp(synthetic_sd, prefix, emb, return_activations=True)
        cut = lambda v: v.reshape(-1, 32, v.shape[-1])
        orders = {h: dk.uor.match(dk.uor.co_dead_counts(cal[key][1][h]).numpy()) for h in dk.uor.RELU_FED}
        want = dk.count(cut(raw), {k: cut(v) for k, v in acts.items()}, key == "coarse", key == "fine", orders)
        assert got[key] == want, key


def test_cli_default_prints_what_tile_rays_1_prints(monkeypatch):
    outs = []
    for extra in ([], ["--tile-rays", "1"]):
        monkeypatch.setattr(sys, "argv", ["dead_ksteps.py", "--rays", "8", "--seed", "5"] + extra)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            assert dk.main() == 0
        outs.append(buf.getvalue())
    assert outs[0] == outs[1] and "rays=8 seed=5; a full tile issues 7680 + 576 MFMAs" in outs[0]
    monkeypatch.setattr(sys, "argv", ["dead_ksteps.py", "--rays", "8", "--seed", "5", "--tile-rays", "4"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert dk.main() == 0
    assert "tile=4 rays x 8 samples" in buf.getvalue()
    monkeypatch.setattr(sys, "argv", ["dead_ksteps.py", "--tile-rays", "3"])
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        dk.main()


@pytest.mark.parametrize("R", SHAPES)
@pytest.mark.parametrize("S", [64, 192])
def test_regrouping_is_a_permutation_into_r_by_s_tiles(R, S):
    """Every point lands in exactly one slot, and tile T holds rays g R .. g R + R - 1 by samples c s .. c s + s - 1 with
    g = T // q, c = T % q, lane slot j -> (ray g R + j // s, sample c s + j % s): the kernel's mapping."""
    n, s = 64, 32 // R
    ray = torch.arange(n).repeat_interleave(S)
    smp = torch.arange(S).repeat(n)
    x = torch.stack([ray, smp], -1)
    tiles = dk.regroup(x, n, S, R)
    assert tiles.shape == (n * S // 32, 32, 2)
    ids = tiles[..., 0] * S + tiles[..., 1]
    assert torch.equal(ids.reshape(-1).sort().values, torch.arange(n * S))
    q = S // s
    T = torch.arange(n * S // 32)[:, None]
    j = torch.arange(32)[None, :]
    assert torch.equal(tiles[..., 0], (T // q) * R + j // s)
    assert torch.equal(tiles[..., 1], (T % q) * s + j % s)


def test_pixel_runs_are_consecutive_pixels_of_one_row():
    for R in SHAPES:
        ids = dk.pixel_runs(64, 0, R).reshape(-1, R)
        assert torch.equal(ids, ids[:, :1] + torch.arange(R))
        assert torch.all(ids[:, 0] // 800 == ids[:, -1] // 800)
        assert ids.unique().numel() == 64


def test_base_family_shaped_tiles_leave_fewer_mfmas(oracle, synthetic_sd):
    """128 rays in runs of 8 consecutive pixels, unit orders from 16 scattered rays on one-ray tiles (the library's rule): tiles of
    4 and of 8 rays leave fewer MFMAs than one-ray tiles of the same rays, in the coarse and in the fine launch, and the colour
    branch runs in no more fine tiles."""
    sd = oracle.weight_family(synthetic_sd, "base")
    res = {R: dk.probe(sd, n_rays=128, seed=0, calibrate_rays=16, tile_rays=R, run_rays=8) for R in (1, 4, 8)}
    for key in ("coarse", "fine"):
        left = {R: res[R][key]["mfma_left_repaired"] for R in res}
        print(key, {R: round(v, 1) for R, v in left.items()})
        assert left[4] < left[1] and left[8] < left[1], (key, left)
        assert res[4][key]["tiles"] == res[1][key]["tiles"]
    assert res[4]["fine"]["colour_live"] <= res[1]["fine"]["colour_live"]
