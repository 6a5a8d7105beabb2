"""-m gpu: the fp16 kernels on real networks against their own rounding floor.  E = f16_reference.emulate is a float64 restatement of
the kernels' arithmetic (same rounding points, another summation order), T = truth16 the network with fp16 weights in float64.
Three criteria per case (four networks x two fp16 precisions), none with a constant measured on the kernel:
  (i)   at least half of the points have all four outputs within the order-free fp32 head bound (K + 2) u (sum|w h| + |b|) of E:
        wherever no hidden-layer rounding flipped, kernel and emulation differ by the heads' summation order only.  0.5 is a cap:
        E against its own fp32-accumulating realisation stays at 0.76-0.82 (tests/test_f16_reference_cpu.py asserts >= 0.7);
  (ii)  no output further than 2 M_c from E, M_c = max_p |E - T|: both are realisations of one rounding process around T;
  (iii) rms_p(gpu - T) <= 1.25 rms_p(E - T) per channel: the same amount of noise (round-toward-zero gives 1.2-18x).
tests/test_f16_reference_cpu.py shows that a dropped tile bias, a truncating conversion and two swapped k-slots each fail them.
Position invariance: in a 131 917-point arrangement of 1024 of the points every copy returns the bits of its first copy."""
import functools

import pytest
import torch

import f16_reference as R
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _points():
    return R.floor_points()


_REFERENCE = {}


def _reference(family_sd, family, prefix):
    """(state dict, E, T, head magnitudes) of one network, computed on the CPU once and left unchanged."""
    if (family, prefix) not in _REFERENCE:
        torch.set_num_threads(8)
        sd = family_sd(family)
        pts, vd = _points()
        E = R.emulate(sd, prefix, pts, vd)
        _REFERENCE[family, prefix] = (sd, E["raw"], R.truth16(sd, prefix, pts, vd), R.head_magnitude(sd, prefix, E))
    return _REFERENCE[family, prefix]


@pytest.mark.parametrize("precision", ["f16", "f16m32"])
@pytest.mark.parametrize("family,prefix", R.FLOOR_CASES)
def test_f16_forward_sits_on_its_rounding_floor(amd, family_sd, family, prefix, precision):
    sd, E, T, mag = _reference(family_sd, family, prefix)
    pts, vd = _points()
    net = amd.Network()
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    net.precision = precision
    model = R.model_of(prefix)
    pts_g, vd_g = pts.cuda(), vd.cuda()
    raw = net.forward(pts_g[:, None, :].contiguous(), vd_g, None, model=model)[:, 0]
    fig = R.floor_figures(raw.cpu(), E, T, mag)
    print(family, prefix, precision, fig)
    R.parity_record("gpu_floor", f"{family}/{prefix}/{precision}", fig)
    assert fig["share"] >= 0.5, fig
    assert max(fig["max_over_M"]) <= 2.0, fig
    assert max(fig["rms_ratio"]) <= 1.25, fig
    # position invariance over many tiles per workgroup
    ids = R.repeated(R.N_MANY, 1024, 11).cuda()
    many = net.forward(pts_g[ids][:, None, :].contiguous(), vd_g[ids].contiguous(), None, model=model)[:, 0]
    first = torch.argsort(ids[:1024])                     # the first 1024 rows are one permutation: where each point stands first
    assert torch.equal(many, many[first[ids]])
