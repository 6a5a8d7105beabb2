"""Helpers that two or more of the GPU test modules share (test infrastructure).  The modules reach the C ABI through the package's
checked path, `amd._lib.call(name, *args)`; only their refusal probes, which need the raw status of deliberately malformed
arguments, assemble ctypes calls by hand."""
import pytest
import torch


@pytest.fixture(scope="module")
def amd():
    import nerf_replication_amd as pkg
    pkg._lib.load()
    return pkg


def network(amd, sd, precision="f32", train=False, frozen=False):
    """amd.Network with the weights of `sd` on the GPU, in train() or eval() mode, optionally with frozen parameters."""
    net = amd.Network()
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    net.train() if train else net.eval()
    if frozen:
        net.requires_grad_(False)
    net.precision = precision
    return net


def rel(got, ref):
    """Largest deviation relative to the reference's largest magnitude, in float64 on the CPU."""
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-9)).item()


def assert_grads_equal(got, ref, bound=1e-4):
    """The project's form and bound for regrouped atomic accumulation of identical terms: relative 1e-4 of the tensor's maximum,
    exact zeros where the reference step has zeros.  -> the largest relative deviation."""
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.isfinite(a).all(), i
        if b.abs().max() == 0:
            assert torch.all(a == 0), i
        else:
            worst = max(worst, rel(a, b))
            assert rel(a, b) <= bound, (i, rel(a, b))
    return worst


class Replay:
    """Renderer._rand replacement that hands out recorded draws in order (and records the shapes asked for)."""

    def __init__(self, draws):
        self.draws, self.shapes = [t for t in draws if t is not None], []

    def __call__(self, shape, device):
        self.shapes.append(tuple(shape))
        t = self.draws.pop(0)
        assert tuple(t.shape) == tuple(shape)
        return t.to(device)
