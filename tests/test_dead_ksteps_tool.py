"""tools/dead_ksteps.py, the CPU probe behind the dead k-step skipping of the fp32 inference kernels: the pairing it uses is the
layout's, its fractions are fractions, and with nothing dead it counts the MFMAs csrc/nerf_layout.h lays out."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import dead_ksteps as dk  # noqa: E402


def test_pairing_is_the_layouts():
    """One activation register holds feature f (bit 2 clear, lane half 0) and f + 4 (lane half 1); the 128 k-steps cover the
    256 features once; k-step 4 g + q is row q of group g as gemm_tiles walks them."""
    pairs = dk.kstep_pairs()
    assert pairs.shape == (128, 2)
    assert torch.all(pairs[:, 0] & 4 == 0) and torch.all(pairs[:, 1] == pairs[:, 0] + 4)
    assert sorted(pairs.reshape(-1).tolist()) == list(range(256))
    from pack_reference import act_feat
    for g in range(32):
        for q in range(4):
            assert pairs[4 * g + q].tolist() == [act_feat(g >> 2, (g & 3) * 4 + q, 0), act_feat(g >> 2, (g & 3) * 4 + q, 1)]


def test_dead_rule_on_a_made_up_tile():
    """Dead = both features zero at all 32 points; one positive value anywhere in the pair, or a NaN, keeps the k-step."""
    h = torch.zeros(3, 32, 256)
    h[0, 31, 4] = 1.0                      # partner of feature 0, last point
    h[1, 0, 250] = float("nan")
    dead = dk.dead_ksteps(h)
    pairs = dk.kstep_pairs().tolist()
    assert dead[2].all() and dead[0].sum() == 127 and dead[1].sum() == 127
    assert not dead[0, pairs.index([0, 4])] and not dead[1, pairs.index([250, 254])]


def test_probe_on_the_synthetic_checkpoint(synthetic_sd):
    """64 rays of the bench frame: fractions lie in [0, 1], skipped MFMAs never exceed issued ones, the coarse pass has no colour
    branch, and the figures have the order of magnitude the kernel change was sized on (fine pass: more than 5 % of the MFMAs)."""
    res = dk.probe(synthetic_sd, n_rays=64, seed=0)
    trunk, colour = dk.layout_mfmas()
    assert (trunk, colour) == (7680, 576)
    assert res["coarse"]["tiles"] == 64 * 2 and res["fine"]["tiles"] == 64 * 6
    for key in ("coarse", "fine"):
        r = res[key]
        for row in r["rows"]:
            for f in (row["feature_off"], row["kstep_dead"]):
                assert f is None or 0.0 <= f <= 1.0
            assert (row["kstep_dead"] is None) == ("PE" in row["gemm"])
            assert 0.0 <= row["mfma_left"] <= row["mfma"] <= row["ksteps"] * row["ntiles"]
            if row["kstep_dead"] is not None and row["feature_off"] is not None:
                assert row["kstep_dead"] <= row["feature_off"] + 1e-12          # a dead pair needs both features off
        assert r["mfma_left"] <= r["mfma"]
    assert res["coarse"]["mfma"] == trunk and len(res["coarse"]["rows"]) == 9
    assert res["fine"]["mfma"] <= trunk + colour and 0.0 < res["fine"]["colour_live"] <= 1.0
    assert res["fine"]["mfma_left"] < 0.95 * res["fine"]["mfma"]


def test_nothing_dead_gives_the_layouts_total():
    """Strictly positive activations: every k-step runs, and a live tile issues what the two weight streams of
    csrc/nerf_layout.h hold -- 4 MFMAs per 1-KiB block: 7680 in the trunk, 576 in the folded colour branch."""
    acts = {f"h{i}": torch.ones(2, 32, 256) for i in range(8)}
    raw = torch.ones(2, 32, 4)
    trunk, colour = dk.layout_mfmas()
    full = dk.count(raw, acts, density_only=False, skip_dead_colour=True)
    dens = dk.count(raw, acts, density_only=True, skip_dead_colour=False)
    assert full["mfma"] == full["mfma_left"] == trunk + colour == sum(k * n for _, k, n, _, _ in dk.GEMMS)
    assert dens["mfma"] == dens["mfma_left"] == trunk
    raw[1, :, 3] = -1.0                    # a tile without density skips the colour branch (DSKIP)
    half = dk.count(raw, acts, density_only=False, skip_dead_colour=True)
    assert half["mfma"] == trunk + colour / 2 and half["colour_live"] == 0.5
