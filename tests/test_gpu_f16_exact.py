"""-m gpu: exact probes of the MLP kernels.  On the networks and points of tests/f16_reference.py every product and every partial
sum is a multiple of 1/4 below 512 (tests/test_f16_reference_cpu.py), so the fp16, the split-fp16 and the fp32 kernels must all
return the CPU float64 result BIT FOR BIT, whatever their summation order: no tolerance, no exempt element.  "f32" and "f32x" are
the controls (their forward is pinned elsewhere); a mismatch in an fp16 precision alone is the fp16 kernel or its pack, and the
failure message names the first mismatching (point, channel) for the layout (csrc/nerf_layout.h, tests/pack_reference.py).

Shapes: the fp16 tile is 256 points and the grid min(tiles, CUs) persistent workgroups -- n = 1, 31, 33, 255, 257 (clamped lanes, a
ragged wave, a ragged tile), the ragged-mask path, 131 917 points (every workgroup walks two or three tiles: stream wrap-around,
the next tile's encoding under the previous tile's views layer, a ragged last tile), and the ray entry with the shared depth table
and with per-ray depths."""
import functools

import pytest
import torch

import f16_reference as R
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu

N_DISTINCT = 1024


@functools.lru_cache(maxsize=None)
def _case(seed, zero_axis):
    """Everything of one probe network that the CPU computes, once: the state dict, 1024 distinct points with their float64 results,
    and the two ray calls with theirs (evaluated on the distinct (point, direction) pairs only)."""
    torch.set_num_threads(8)
    sub = R.probe_network(seed, zero_axis)
    pts, dirs = R.probe_points(seed, zero_axis, N_DISTINCT)
    want = R.probe_forward(sub, pts, dirs)
    gen = torch.Generator().manual_seed(31 * seed + zero_axis)
    rays = {}
    for name, n_rays, S, per_ray in (("shared", 3, 64, False), ("per_ray", 700, 192, True)):
        o, d, t, rpts, unit = R.probe_rays(gen, zero_axis, n_rays, S, per_ray)
        rows = torch.cat([rpts, unit[:, None, :].expand(n_rays, S, 3)], -1).reshape(-1, 6)
        uniq, inverse = torch.unique(rows, dim=0, return_inverse=True)
        up, ud = uniq[:, :3].contiguous(), uniq[:, 3:].contiguous()
        rwant = R.probe_forward(sub, up, ud)
        assert torch.equal(R.probe_forward(sub, up, ud, torch.float32), rwant)     # these points are exact too
        rays[name] = (o, d, t, rwant[inverse].reshape(n_rays, S, 4))
    mask = torch.rand(257, generator=gen) < 0.4
    return dict(sd=R.both_models(sub), pts=pts, dirs=dirs, want=want, rays=rays, mask=mask, many=R.repeated(R.N_MANY, N_DISTINCT, 5 + seed))


def _same(got, want, what, tally):
    """torch.equal; a mismatch goes to tally["failures"] with its pattern, so that one run shows every call that disagrees."""
    want = want.to(got.device)
    tally["points"] += got.numel() // 4
    if torch.equal(got, want):
        return
    bad = (got != want).reshape(-1, 4)
    first = bad.any(-1).nonzero()[0].item()
    tally["mismatching_points"] += int(bad.any(-1).sum())
    tally["failures"].append(f"{what}: {int(bad.any(-1).sum())} of {bad.shape[0]} points differ (per channel {bad.sum(0).tolist()}); first at point {first}: "
                             f"got {got.reshape(-1, 4)[first].tolist()}, want {want.reshape(-1, 4)[first].tolist()}")


@pytest.mark.parametrize("precision", ["f16", "f16m32", "f32x", "f32"])
@pytest.mark.parametrize("seed,zero_axis", R.PROBES)
def test_exact_probe(amd, seed, zero_axis, precision):
    c = _case(seed, zero_axis)
    L = amd._lib
    net = amd.Network()
    net.load_state_dict(c["sd"], strict=True)
    net = net.cuda().eval()
    net.precision = precision
    prec = L.PRECISIONS[precision]
    pts, dirs, want = c["pts"].cuda(), c["dirs"].cuda(), c["want"].cuda()
    tag = f"{precision} seed {seed} axis {zero_axis}"
    tally = dict(points=0, mismatching_points=0, failures=[])
    for model in ("", "fine"):
        for n in (1, 31, 33, 255, 257):
            raw = net.forward(pts[:n, None, :].contiguous(), dirs[:n].contiguous(), None, model=model)
            _same(raw[:, 0], want[:n], f"{tag} forward[{model or 'coarse'}] n={n}", tally)
    mask = c["mask"].cuda()
    raw = net.forward(pts[:257, None, :].contiguous(), dirs[:257].contiguous(), mask[:, None], model="fine")[:, 0]
    masked_out_zero = bool(torch.all(raw[~mask] == 0))
    _same(raw[mask], want[:257][mask], f"{tag} masked forward n=257", tally)
    many = c["many"].cuda()
    raw = net.forward(pts[many][:, None, :].contiguous(), dirs[many].contiguous(), None, model="fine")
    _same(raw[:, 0], want[many], f"{tag} forward[fine] n={R.N_MANY}", tally)
    for (name, (o, d, t, rwant)), model in zip(c["rays"].items(), ("", "fine")):
        n_rays, S = rwant.shape[:2]
        o, d, t = o.cuda(), d.cuda(), t.cuda()
        out = torch.full((n_rays, S, 4), float("nan"), device="cuda")
        L.call("nerf_mlp_forward_rays", o, d, t, S if t.dim() == 2 else 0, n_rays, S, net.packed(model), out, prec)
        torch.cuda.synchronize()
        _same(out, rwant, f"{tag} nerf_mlp_forward_rays[{name}]", tally)
    R.parity_record("gpu_exact_probes", f"seed{seed}/axis{zero_axis}/{precision}", dict(points=tally["points"], mismatching_points=tally["mismatching_points"],
                                                                                       masked_out_zero=masked_out_zero))
    assert masked_out_zero
    assert not tally["failures"], "\n".join(tally["failures"])
