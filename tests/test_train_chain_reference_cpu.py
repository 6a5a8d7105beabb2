"""The yardstick of tests/test_gpu_train_chain_exact.py, checked without a GPU (tests/train_chain_reference.py): on all nine probe
networks the hand-written backward equals torch autograd bit for bit, float32 equals float64 on everything the GPU test compares,
the any-order conditions hold, both mask conventions are exercised -- and each seeded fault changes a compared integer."""
import functools

import pytest
import torch

import f16_reference as R
import train_chain_reference as T

P_POINTS = 257                                   # nine tiles, the last one ragged
RAYS = (37, 5)                                   # 185 points, per-ray depths


@functools.lru_cache(maxsize=None)
def _case(seed, zero_axis):
    torch.set_num_threads(8)
    sub = R.probe_network(seed, zero_axis)
    pts, dirs = R.probe_points(seed, zero_axis, P_POINTS)
    draw = T.integer_draw(P_POINTS, seed)
    rc = T.ray_case(seed, zero_axis, *RAYS, True)
    rdraw = T.integer_draw(RAYS[0] * RAYS[1], 50 + seed)
    return dict(sub=sub, pts=pts, dirs=dirs, draw=draw, rc=rc, rdraw=rdraw,
                points=T.reference(sub, pts, dirs, draw),
                rays=T.reference(sub, rc["pts"], rc["dirs"], rdraw, n_samples=RAYS[1], rays_d=rc["d"]))


def _autograd(sub, pts, dirs, draw, rays=None):
    """network.py:49-74 under torch autograd in float64, loss = sum(raw * draw) -> what T.reference returns, by the same names."""
    dt = torch.float64
    params = {k: v.to(dt).requires_grad_(True) for k, v in sub.items()}
    out = {}
    if rays is None:
        x = pts.to(dt).requires_grad_(True)
        v = dirs.to(dt).requires_grad_(True)
        leaves = dict(g_x=x, g_v=v)
    else:
        n, S = rays["n_rays"], rays["S"]
        t = rays["t"].to(dt).requires_grad_(True)
        d_view = rays["d"].to(dt).requires_grad_(True)
        x_mid = rays["o"].to(dt)[:, None, :] + rays["d"].to(dt)[:, None, :] * t[:, :, None]
        x = x_mid.reshape(-1, 3)
        x_mid.retain_grad()
        v = (d_view / torch.norm(d_view, dim=-1, keepdim=True))[:, None, :].expand(n, S, 3).reshape(-1, 3)
        leaves = dict(g_t=t, g_rays_d_view=d_view)
    F = T.forward(params, x, v, dt)
    for k in [f"z{l}" for l in range(8)] + ["zv", "feature"]:
        F[k].retain_grad()
    (F["raw"] * draw.to(dt)).sum().backward()
    for l in range(8):
        out[f"gz{l}"] = F[f"z{l}"].grad
    out["gzv"], out["gf"] = F["zv"].grad, F["feature"].grad
    for k, leaf in leaves.items():
        out[k] = leaf.grad
    if rays is not None:
        out["g_x"] = x_mid.grad.reshape(-1, 3)
        out["g_t"] = out["g_t"].reshape(-1)
    out["grads"] = [params[k].grad for k in T.oracle.SUBMODEL_KEYS]
    return out


@pytest.mark.parametrize("seed,zero_axis", R.PROBES)
def test_hand_written_backward_equals_autograd(seed, zero_axis):
    c = _case(seed, zero_axis)
    assert torch.equal(c["points"]["raw"].float(), R.probe_forward(c["sub"], c["pts"], c["dirs"]))
    for ref, auto in ((c["points"], _autograd(c["sub"], c["pts"], c["dirs"], c["draw"])),
                      (c["rays"], _autograd(c["sub"], c["rc"]["pts"], c["rc"]["dirs"], c["rdraw"], c["rc"]))):
        for k, want in auto.items():
            if k == "grads":
                for i, (g, w) in enumerate(zip(ref["grads"], want)):
                    assert torch.equal(g, w), (k, i)
            else:
                assert torch.equal(ref[k], want), k


def _compared(ref, masks, cols):
    """Every tensor the GPU test holds to torch.equal, as a flat {name: tensor}."""
    pe_ok, dpe_ok = cols
    out = {k: ref[k] for k in T.ROW_NAMES + T.SAVE_NAMES[2:] + ["raw", "g_x", "g_v"] if k in ref}
    out["pe"], out["dpe"] = ref["pe"][:, pe_ok], ref["dpe"][:, dpe_ok]
    for k in ("g_t", "g_rays_d_view"):
        if k in ref:
            out[k] = ref[k]
    for i, (g, keep) in enumerate(zip(ref["grads"], masks)):
        out[f"grad{i}"] = g[keep]
    out["bits"] = T.bits_blocks(ref, ref["raw"].shape[0])[0]
    return out


@pytest.mark.parametrize("seed,zero_axis", R.PROBES)
def test_float32_equals_float64_and_the_conditions_hold(seed, zero_axis):
    c = _case(seed, zero_axis)
    masks, cols = T.exact_masks(zero_axis), T.exact_columns(zero_axis)
    assert sum(int((~m).sum()) for m in masks) == T.N_EXEMPT and sum(m.numel() for m in masks) == T.N_GRADIENT
    f32 = dict(points=T.reference(c["sub"], c["pts"], c["dirs"], c["draw"], torch.float32),
               rays=T.reference(c["sub"], c["rc"]["pts"], c["rc"]["dirs"], c["rdraw"], torch.float32, n_samples=RAYS[1], rays_d=c["rc"]["d"]))
    for mode in ("points", "rays"):
        ref = c[mode]
        fig = T.check_conditions(ref, masks)                          # |value|, sum|terms| < 2^24 units; chain values < 2^11
        want, got = _compared(ref, masks, cols), _compared(f32[mode], masks, cols)
        for k in want:
            assert got[k].dtype in (torch.float32, torch.int32)
            assert torch.equal(got[k].double(), want[k].double()), (mode, k)
            if k != "bits":
                assert torch.equal(want[k] * T.GRID, (want[k] * T.GRID).round()) and float(want[k].abs().max()) * T.GRID < T.TWO24, (mode, k)
        sigma = ref["raw"][:, 3]
        assert bool((sigma > 0).any()) and bool((sigma < 0).any())
        for k in [f"z{l}" for l in range(8)] + ["zv"]:                # integer biases: the > against >= convention is exercised
            assert bool((ref[k] == 0).any()), k
            live = float((ref[k] > 0).double().mean())
            assert 0.2 < live < 0.8, (k, live)
        print(f"seed {seed} axis {zero_axis} {mode}: {fig}")


@pytest.mark.parametrize("fault", T.FAULTS)
@pytest.mark.parametrize("seed,zero_axis", R.PROBES)
def test_seeded_fault_changes_a_compared_integer(seed, zero_axis, fault):
    c = _case(seed, zero_axis)
    masks, cols = T.exact_masks(zero_axis), T.exact_columns(zero_axis)
    mode = "rays" if fault == "g_t_unit_direction" else "points"
    if mode == "rays":
        bad = T.reference(c["sub"], c["rc"]["pts"], c["rc"]["dirs"], c["rdraw"], n_samples=RAYS[1], rays_d=c["rc"]["d"], fault=fault)
    else:
        bad = T.reference(c["sub"], c["pts"], c["dirs"], c["draw"], fault=fault)
    want, got = _compared(c[mode], masks, cols), _compared(bad, masks, cols)
    changed = {k: int((got[k] != want[k]).sum()) for k in want if not torch.equal(got[k], want[k])}
    print(f"seed {seed} axis {zero_axis} {fault}: changed elements {changed}")
    assert changed, fault
    rows = {"mask_ge", "mask_other_tile", "alpha_dropped", "w5_parts_swapped", "row_duplicated"}
    assert (fault not in rows) or any(k in changed for k in T.ROW_NAMES), (fault, changed)
    assert fault != "g_t_unit_direction" or set(changed) == {"g_t"}


def test_bit_blocks_decode_as_the_layout_says():
    """bits_blocks against the plain loop over (tile, tensor, lane, feature tile, register) of TrainSave::off_bits."""
    c = _case(0, 0)
    P = 45
    ref = {k: v[:P] for k, v in c["points"].items() if k.startswith("z")}
    words, compared = T.bits_blocks(ref, P)
    assert words.shape == (2, 9, 64, 4) and words.dtype == torch.int32
    for tile in range(2):
        for which, key, ntile in [(0, "z0", 8), (5, "z5", 8), (8, "zv", 4)]:
            for lane in (0, 12, 31, 32, 44, 63):
                pt, hh = lane & 31, lane >> 5
                p = 32 * tile + pt
                assert bool(compared[tile, which, lane, 0]) == (p < P)
                assert bool(compared[tile, which, lane, 3]) == (p < P and ntile == 8)
                if p >= P:
                    continue
                for t in range(ntile):
                    for r in range(16):
                        feat = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh
                        bit = (int(words[tile, which, lane, t >> 1]) >> (16 * (t & 1) + r)) & 1
                        assert bit == int(ref[key][p, feat] > 0), (tile, which, lane, t, r)
    dens = T.bits_blocks(ref, P, density_only=True)[1]
    assert not bool(dens[:, 8].any()) and bool(dens[:, 7, 0].all())


def test_dead_tile_arrangement_and_liveness():
    c = _case(1, 1)
    pts, dirs = R.probe_points(1, 1, 1024)
    sigma = T.forward(c["sub"], pts, dirs)["raw"][:, 3]
    for P, n_dead in ((160, 2), (192, 3)):
        ids = T.arrange_dead_tiles(sigma, P, n_dead)
        assert ids.shape == (P,) and len(set(ids.tolist())) == P
        s = sigma[ids].view(-1, 32)
        assert bool((s[:n_dead] <= 0).all()) and bool((s[n_dead:] > 0).any(-1).all()) and bool((s[n_dead:] <= 0).any(-1).all())
        draw = T.integer_draw(P, 3) * (sigma[ids] > 0)[:, None]
        flags, count = T.tile_liveness(draw)
        assert count == P // 32 - n_dead and flags.tolist() == [False] * n_dead + [True] * (P // 32 - n_dead)
    assert T.n_many(256) == 2 * 128 * 256 + 3 * 128 + 77
    for P, (n, S) in T.RAY_SHAPES.items():
        assert n * S == P
