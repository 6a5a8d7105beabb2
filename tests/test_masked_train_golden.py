"""CPU: the fixture of the masked / coarse-only training steps (tests/golden/masked_train.npz, the REAL reference under
autograd, tools/gen_masked_train_golden.py) against the oracle under autograd.  This guards the fixture the GPU tests of
tests/test_gpu_masked_training.py are judged by; it does not touch the HIP path."""
import pytest
import torch

from train_steps_common import subsample

GRAD_STRIDE = 53
MASKED_CASES = (("trained_t002", "trained", 0.02), ("sharp_t025", "sharp", 0.25), ("trained_t025", "trained", 0.25))


def _case(golden, tag):
    g = golden("masked_train.npz")
    assert int(g["grad_stride"]) == GRAD_STRIDE
    return g, {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + "/")}


def _check_grads(sd, c, prefixes):
    """fp32 noise: the bound of test_oracle_golden.test_autograd_fixture (rtol 1e-4, atol 1e-6), with the absolute term taken
    relative to the tensor's largest entry -- the masked reference compacts the valid points before its MLP chunks, so its GEMM
    row grouping, hence the summation order of every weight gradient, differs from the oracle's."""
    n = 0
    for k, v in sd.items():
        if not k.startswith(prefixes):
            assert v.grad is None, k
            continue
        ref = c["grad/" + k]
        got = subsample(v.grad, GRAD_STRIDE)
        assert got.shape == ref.shape, k
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-6 + 1e-5 * ref.abs().max().item()), (k, (got - ref).abs().max().item(), ref.abs().max().item())
        n += 1
    return n


@pytest.mark.parametrize("tag,family,thr", MASKED_CASES)
def test_oracle_reproduces_the_masked_step(oracle, golden, family_sd, tag, family, thr):
    g, c = _case(golden, tag)
    assert float(c["weights_threshold"]) == pytest.approx(thr) and float(g["amplitude_rel"]) == pytest.approx(2.3e-5)
    assert c["rays_o"].shape == (96, 3) and c["amplitude"] > 0
    o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(40.0), pixel_ids=c["pixel_ids"])
    assert torch.equal(o, c["rays_o"]) and torch.equal(d, c["rays_d"])
    sd = {k: v.clone().requires_grad_(True) for k, v in family_sd(family).items()}
    rgb, dep, parts = oracle.render(sd, o[None], d[None], fast_sampling=True, weights_threshold=thr, return_parts=True)
    # the mask, bit for bit, and what it is made from
    assert torch.equal(parts["raw_coarse"][..., 3].detach(), c["sigma_coarse_raw"])
    assert torch.equal(parts["t_sorted"].detach(), c["t_sorted"])
    assert torch.equal(parts["valid_sorted"], c["valid_sorted"].bool())
    t_c = oracle.stratified_t().expand(96, 64)
    vf = oracle.fine_valid_mask(torch.relu(c["sigma_coarse_raw"]), t_c, weights_threshold=thr)
    assert torch.equal(vf, c["valid_fine"].bool())
    assert int(parts["valid_sorted"].sum()) == 64 * 96 + int(c["valid_fine"].sum())
    if tag == "trained_t025":
        assert int(c["valid_fine"].sum()) == 0                       # no fine sample valid: M = 64 n
    else:
        assert 0.1 < c["valid_fine"].float().mean() < 0.6
    # image and loss: the bounds of test_ess_ert_masked_path
    assert (rgb.detach() - c["rgb"]).abs().max() <= 1e-6 and (dep.detach() - c["depth"]).abs().max() <= 1e-5
    loss = torch.nn.functional.mse_loss(rgb, c["target"])
    assert abs(loss.item() - c["loss"].item()) <= 1e-6 * max(1.0, abs(c["loss"].item()))
    loss.backward()
    assert _check_grads(sd, c, ("model.", "model_fine.")) == 48
    assert sum(v.grad.abs().sum() for k, v in sd.items() if k.startswith("model.")) > 0
    for k in ("model.rgb_linear.weight", "model.views_linears.0.weight", "model.feature_linear.weight"):
        assert torch.all(c["grad/" + k] == 0), k


def test_oracle_reproduces_the_coarse_only_step(oracle, golden, family_sd):
    _, c = _case(golden, "coarse_only")
    o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(40.0), pixel_ids=c["pixel_ids"])
    assert torch.equal(o, c["rays_o"]) and torch.equal(d, c["rays_d"])
    sd = {k: v.clone().requires_grad_(True) for k, v in family_sd("trained").items()}
    rgb, dep, parts = oracle.render(sd, o[None], d[None], n_importance=0, return_parts=True)
    assert torch.equal(parts["raw_coarse"][..., 3].detach(), c["sigma_coarse_raw"])
    assert torch.equal(rgb.detach(), c["rgb"]) and torch.equal(dep.detach(), c["depth"])
    loss = torch.nn.functional.mse_loss(rgb, c["target"])
    assert torch.equal(loss.detach(), c["loss"])
    loss.backward()
    assert _check_grads(sd, c, ("model.",)) == 24
    assert not any(k.startswith("grad/model_fine.") for k in c)


def test_fixture_is_small_and_holds_its_selection_parameters(golden):
    import os
    from conftest import GOLDEN
    g = golden("masked_train.npz")
    assert os.path.getsize(os.path.join(GOLDEN, "masked_train.npz")) < (1 << 20)
    assert int(g["stability_draws"]) == 8 and int(g["seed"]) == 11
