"""Generate the stochastic-sampling fixtures tests/golden/stochastic_*.npz by running the REAL reference on CPU.

The reference's training sampling mode (Renderer.task == "train", perturb on) draws torch.rand twice per render call:
the coarse jitter [n,64] (volume_renderer.py:59) and the inverse-CDF u [n,128] (:145).  This script sets that mode on the
reference's own Renderer, seeds torch, and records every torch.rand draw by wrapping torch.rand for the duration of the
call; the fixtures hold those draws next to the inputs and outputs, so the tests replay them (Renderer._rand).  Like
oracle/gen_golden.py (whose import recipe, npz writer and ray helpers it imports) it needs the reference checkout and runs
in the build container only; no reference source is copied.

    python tools/gen_stochastic_golden.py        # rewrites the two files below, bit-identically

  stochastic_render.npz        no-grad renders of 160 pinhole rays each: the trained checkpoint ("trained") and the sharp
                               synthetic family ("sharp") with jitter + random u, and the trained checkpoint with perturb
                               off (random u alone, "trained_u").  Per run: rays, draws, coarse sigma (pre-ReLU), the merged
                               depths t_sorted, rgb, depth.
  stochastic_train_steps.npz   K = 5 reference training steps (render under autograd, MSE, backward, clip 40, Adam 5e-4) on
                               96 pinhole rays from the trained checkpoint (teacher: the sharp family), fresh draws every
                               step.  Per step: the draws and the loss; step 1: rgb, depth, coarse sigma and the gradients (flat stride-17 subsample of the
                               weight matrices); step K: the parameters (stride-31 subsample).  The strides keep the file
                               under 1 MiB; both are coprime to every row length (63, 128, 256, 283, 319).
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import gen_golden as gg  # noqa: E402  (import_reference, npz, OUT)
import nerf_oracle as orc  # noqa: E402

K_STEPS = 5
N_RENDER = 160
N_TRAIN = 96


class RecordRand:
    """Wrap torch.rand while active: every draw is passed through and a copy kept in `calls` (in call order)."""

    def __enter__(self):
        self.calls, self._orig = [], torch.rand

        def rand(*args, **kwargs):
            t = self._orig(*args, **kwargs)
            self.calls.append(t.detach().clone())
            return t
        torch.rand = rand
        return self

    def __exit__(self, *exc):
        torch.rand = self._orig
        return False


class ReplayRand:
    """torch.rand returns the given tensors in order while active (re-derivation of the reference's intermediates)."""

    def __init__(self, draws):
        self.draws = list(draws)

    def __enter__(self):
        self._orig = torch.rand
        torch.rand = lambda *a, **k: self.draws.pop(0).clone()
        return self

    def __exit__(self, *exc):
        torch.rand = self._orig
        assert not self.draws, "unused draws"
        return False


def _subsample(t, stride):
    f = t.detach().reshape(-1)
    return f.clone() if f.numel() <= 4096 else f[::stride].clone()


def _net(Network, sd, train):
    net = Network()
    net.load_state_dict({k: sd[k].clone() for k in orc.state_dict_keys()}, strict=True)
    net.train() if train else net.eval()
    return net


def _stochastic(ren, perturb):
    ren.device = torch.device("cpu")
    ren.task = "train"
    ren.perturb = perturb
    return ren


def render_fixtures(Network, Renderer, base, trained):
    ids = torch.from_numpy(np.random.default_rng(5).choice(800 * 800, N_RENDER, replace=False))
    o, d = orc.pinhole_rays(800, 800, orc.camera_pose(70.0), pixel_ids=ids)
    runs = (("trained", trained, True), ("sharp", orc.weight_family(base, "sharp"), True), ("trained_u", trained, False))
    rec = {"rays_o": o, "rays_d": d}
    for seed, (tag, sd, perturb) in enumerate(runs):
        net = _net(Network, sd, train=False)
        ren = _stochastic(Renderer(net), perturb)
        torch.manual_seed(100 + seed)
        with torch.no_grad():
            with RecordRand() as rr:
                rgb, dep = ren.render({"rays_o": o[None], "rays_d": d[None]})
            shapes = [tuple(c.shape) for c in rr.calls]
            assert shapes == ([(N_RENDER, 64)] if perturb else []) + [(N_RENDER, 128)], shapes
            # the reference's own methods on the recorded draws: the coarse sigma and the merged depths of this render
            with ReplayRand(rr.calls[:-1]):
                t_c, pts_c = ren.stratified_sample_points_from_rays(o, d, N_samples=64, perturb=perturb)
            vd = d / torch.norm(d, dim=-1, keepdim=True)
            raw_c = net.forward(pts_c, vd, None, model="")
            with ReplayRand(rr.calls[-1:]):
                _, t_f, vm = ren.fine_sample_points(torch.relu(raw_c[..., 3]), o, d, t_c, 128, 64, 0.25)
            assert vm is None
            t_sorted, _ = torch.sort(torch.cat([t_c, t_f], 1), dim=-1)
        if perturb:
            rec[f"{tag}_jitter"] = rr.calls[0]
        rec.update({f"{tag}_u": rr.calls[-1], f"{tag}_sigma_coarse_raw": raw_c[..., 3], f"{tag}_t_sorted": t_sorted,
                    f"{tag}_rgb": rgb, f"{tag}_depth": dep})
        print(f"  [{tag}] mean rgb {rgb.mean().item():.6f}")
    gg.npz("stochastic_render.npz", **rec)


def train_fixtures(Network, Renderer, base, trained):
    ids = torch.from_numpy(np.random.default_rng(7).choice(800 * 800, N_TRAIN, replace=False))
    o, d = orc.pinhole_rays(800, 800, orc.camera_pose(40.0), pixel_ids=ids)
    teacher = _net(Network, orc.weight_family(base, "sharp"), train=False)
    t_ren = Renderer(teacher)
    t_ren.device = torch.device("cpu")
    assert t_ren.perturb is False and t_ren.task != "train"
    with torch.no_grad():
        target, _ = t_ren.render({"rays_o": o[None], "rays_d": d[None]})
    net = _net(Network, trained, train=True)
    ren = _stochastic(Renderer(net), True)
    # the optimizer of src/train/optimizer.py:8-28 as lego.yaml configures it (gen_golden.training_fixtures asserts the same)
    opt = torch.optim.Adam([{"params": [p], "lr": 5e-4, "weight_decay": 0.0, "eps": 1e-8} for p in net.parameters()],
                           5e-4, weight_decay=0.0, eps=1e-8)
    crit = torch.nn.MSELoss()
    rec = {"rays_o": o, "rays_d": d, "pixel_ids": ids, "target": target, "K": K_STEPS}
    losses, jit, us = [], [], []
    torch.manual_seed(200)
    for step in range(1, K_STEPS + 1):
        with RecordRand() as rr:
            rgb, dep = ren.render({"rays_o": o[None], "rays_d": d[None]})
        assert [tuple(c.shape) for c in rr.calls] == [(N_TRAIN, 64), (N_TRAIN, 128)]
        jit.append(rr.calls[0])
        us.append(rr.calls[1])
        loss = crit(rgb, target)
        opt.zero_grad()
        loss.backward()
        if step == 1:
            with torch.no_grad(), ReplayRand(rr.calls[:1]):
                _, pts_c = ren.stratified_sample_points_from_rays(o, d, N_samples=64, perturb=True)
                vd = d / torch.norm(d, dim=-1, keepdim=True)
                rec["sigma_coarse_raw_step1"] = net.forward(pts_c, vd, None, model="")[..., 3].clone()
            rec["rgb_step1"], rec["depth_step1"] = rgb.detach().clone(), dep.detach().clone()
            for k, p in net.named_parameters():
                rec["grad1/" + k] = _subsample(p.grad, 17)
        torch.nn.utils.clip_grad_value_(net.parameters(), 40)
        opt.step()
        losses.append(loss.detach().clone())
        print(f"  [train] step {step}: loss {loss.item():.8f}")
    for k, p in net.named_parameters():
        rec[f"param{K_STEPS}/" + k] = _subsample(p, 31)
    rec["loss"] = torch.stack(losses)
    rec["jitter"] = torch.stack(jit)            # [K, n, 64]
    rec["u"] = torch.stack(us)                  # [K, n, 128]
    gg.npz("stochastic_train_steps.npz", **rec)


def main():
    torch.set_num_threads(8)
    Network, Renderer = gg.import_reference()
    base = torch.load(os.path.join(gg.OUT, "synthetic_ckpt.pth"), weights_only=True)["net"]
    base = {k: base[k] for k in orc.state_dict_keys()}
    trained = torch.load(os.path.join(gg.OUT, "trained_ckpt.pth"), weights_only=True)["net"]
    render_fixtures(Network, Renderer, base, trained)
    train_fixtures(Network, Renderer, base, trained)


if __name__ == "__main__":
    main()
