"""CPU checks of tests/f16_reference.py, the yardstick of the fp16 GPU tests: the exact probes really are exact (so a bit-for-bit
comparison on the GPU is a fair demand in every precision), the two realisations of the fp16 emulation agree as closely as the GPU
criteria assume, and every seeded fault is caught by those criteria (so they can fail).  Figures go to profiles/f16_parity.json."""
import functools

import pytest
import torch

import f16_reference as R
import nerf_oracle as oracle

N_PROBE = 1024


@pytest.mark.parametrize("seed,zero_axis", R.PROBES)
def test_probe_is_exact_and_alive(seed, zero_axis):
    sub = R.probe_network(seed, zero_axis)
    pts, dirs = R.probe_points(seed, zero_axis, N_PROBE)
    assert set(sub) == set(oracle.SUBMODEL_KEYS) and all(sub[k].shape == oracle.SUBMODEL_SHAPES[k] for k in sub)
    for k, v in sub.items():
        nnz = (v != 0).sum(-1)
        if k.endswith("weight"):
            want = 8 if k.startswith(("alpha", "rgb")) else 4
            assert torch.all(nnz == want) and torch.all(v.sum(-1) == 0) and torch.all(v.abs() <= 1)
        elif not k.startswith("alpha"):
            assert torch.all(v == v.round()) and v.abs().max() <= 2
    W = lambda n: sub[n + ".weight"].double()
    B = lambda n: sub[n + ".bias"].double()
    pe = oracle.freq_encode(pts.double(), oracle.XYZ_FREQS)
    de = oracle.freq_encode(dirs.double(), oracle.DIR_FREQS)
    grid = lambda x: bool(torch.all(x * 4 == (x * 4).round()) and x.abs().max() <= 512)
    live = {}

    def dense(x, name):
        used = (W(name) != 0).any(0)
        assert grid(x[:, used]), f"{name}: an input that meets a non-zero weight is off the 1/4 grid"
        z = x @ W(name).T + B(name)
        assert grid(z), f"{name}: pre-activation off the 1/4 grid or above 512"
        assert (x.abs() @ W(name).abs().T + B(name).abs()).max() < 2 ** 24
        return z

    h = pe
    for i in range(8):
        h = torch.relu(dense(h, f"pts_linears.{i}"))
        live[f"pts_linears.{i}"] = (h > 0).double().mean().item()
        if i == 4:
            h = torch.cat([pe, h], -1)
    sigma = dense(h, "alpha_linear")
    hv = torch.relu(dense(torch.cat([dense(h, "feature_linear"), de], -1), "views_linears.0"))
    live["views_linears.0"] = (hv > 0).double().mean().item()
    raw = torch.cat([dense(hv, "rgb_linear"), sigma], -1)
    r64 = R.probe_forward(sub, pts, dirs, torch.float64)
    assert torch.equal(r64.double(), raw)                                   # the oracle in float64 is this walk
    assert torch.equal(R.probe_forward(sub, pts, dirs, torch.float32), r64)      # and its float32 evaluation returns the same bits
    assert all(0.25 <= v <= 0.75 for v in live.values()), live
    pos, nonpos = (sigma > 0).double().mean().item(), (sigma <= 0).double().mean().item()
    assert pos >= 0.1 and nonpos >= 0.1
    distinct = torch.unique(raw, dim=0).shape[0]
    assert distinct >= 256
    # the fp16 emulation itself returns the same bits: every rounding point is exact here
    sd = R.both_models(sub)
    assert torch.equal(R.emulate(sd, "model", pts, dirs)["raw"], raw)
    assert torch.equal(R.emulate(sd, "model", pts, dirs, accumulate=torch.float32)["raw"], raw)
    assert torch.equal(R.emulate(sd, "model", pts, dirs, toward_zero=True)["raw"], raw)         # nothing is rounded, in either mode
    # and the probe sees an addressing fault: one dropped tile bias or two swapped k-slots change whole outputs
    for kw in (dict(drop_bias=("pts_linears.3", 5)), dict(swap_slots=("pts_linears.6", 3, 17)), dict(swap_slots=("views_linears.0", 31, 32))):
        moved = (R.emulate(sd, "model", pts, dirs, **kw)["raw"] != raw).any(-1).double().mean().item()
        assert moved >= 0.25, (kw, moved)
    R.parity_record("cpu_probes", f"seed{seed}/axis{zero_axis}", dict(live_min=min(live.values()), live_max=max(live.values()), sigma_positive=pos,
                                                                     distinct_rows=distinct, max_abs=max(raw.abs().max().item(), h.abs().max().item())))


@functools.lru_cache(maxsize=None)
def _points():
    return R.floor_points()


# the out-tile whose dropped bias each case must catch: the tile of pts_linears.3 with the largest |bias| sum
def _bias_tile(sd, prefix):
    return int(sd[f"{prefix}.pts_linears.3.bias"].abs().reshape(16, 16).sum(-1).argmax())


@pytest.mark.parametrize("family,prefix", R.FLOOR_CASES)
def test_emulation_agrees_with_itself_and_catches_seeded_faults(family_sd, family, prefix):
    torch.set_num_threads(8)
    sd = family_sd(family)
    pts, vd = _points()
    assert pts.shape == (R.N_FLOOR, 3)
    E = R.emulate(sd, prefix, pts, vd)
    T = R.truth16(sd, prefix, pts, vd)
    mag = R.head_magnitude(sd, prefix, E)
    second = R.floor_figures(R.emulate(sd, prefix, pts, vd, accumulate=torch.float32)["raw"], E["raw"], T, mag)
    rec = {"fp32_accumulation": second}
    print(family, prefix, "fp32 accumulation vs float64:", second)
    assert second["share"] >= 0.7, second
    assert max(second["max_over_M"]) <= 2.0, second
    assert max(second["rms_ratio"]) <= 1.25, second
    m = _bias_tile(sd, prefix)
    faults = {f"drop_bias/pts_linears.3/tile{m}": dict(drop_bias=("pts_linears.3", m)), "round_toward_zero": dict(toward_zero=True),
              "swap_slots/pts_linears.6/3<->17": dict(swap_slots=("pts_linears.6", 3, 17))}
    for name, kw in faults.items():
        fig = R.floor_figures(R.emulate(sd, prefix, pts, vd, **kw)["raw"], E["raw"], T, mag)
        verdict = R.floor_verdicts(fig, 0.5)
        rec[name] = dict(fig, caught_by=[k for k, ok in verdict.items() if not ok])
        print(family, prefix, name, fig, verdict)
    R.parity_record("cpu_emulation", f"{family}/{prefix}", rec)
    for name in faults:
        assert rec[name]["caught_by"], (name, rec[name])
