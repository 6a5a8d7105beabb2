#!/usr/bin/env python3
"""Interleaved timing of one training step, deterministic vs stochastic sampling (the reference's task == "train" mode).

    python tools/ab_stochastic_train.py [f32|f32x ...]

Per precision: one Renderer in each mode on the same network, 4096 pinhole rays, train_step (render under autograd, MSE,
backward, FusedAdam) alternated between the two modes for AB_ROUNDS rounds (default 30) of AB_STEPS steps (default 5), HIP
events around each round; medians per step.  The stochastic step includes its two torch.rand draws.  Developer tool."""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import nerf_oracle as orc  # noqa: E402  (pinhole rays only)


def main():
    import nerf_replication_amd as pkg
    from nerf_replication_amd.training import FusedAdam, train_step
    precs = sys.argv[1:] or ["f32", "f32x"]
    rounds, steps = int(os.environ.get("AB_ROUNDS", "30")), int(os.environ.get("AB_STEPS", "5"))
    dev = torch.device("cuda:0")
    ck = torch.load(os.path.join(REPO, "tests", "golden", "trained_ckpt.pth"), weights_only=True)["net"]
    ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(1))[:4096]
    o, d = orc.pinhole_rays(800, 800, orc.camera_pose(30.0), pixel_ids=ids)
    o, d = o.to(dev).contiguous(), d.to(dev).contiguous()
    for prec in precs:
        net = pkg.Network()
        net.load_state_dict({k: ck[k] for k in orc.state_dict_keys()})
        net = net.to(dev).train()
        net.precision = prec
        with torch.no_grad():
            target, _ = pkg.Renderer(net).render({"rays_o": o[None], "rays_d": d[None]})
        det = pkg.Renderer(net)
        sto = pkg.Renderer(net)
        sto.task, sto.perturb = "train", True
        opt = FusedAdam(net.parameters(), lr=1e-6)       # tiny steps: the scene stays put over the measurement
        times = {"deterministic": [], "stochastic": []}
        for rnd in range(rounds + 1):
            for name, ren in (("deterministic", det), ("stochastic", sto)) if rnd % 2 == 0 else (("stochastic", sto), ("deterministic", det)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    train_step(ren, opt, o, d, target)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(e0.elapsed_time(e1) / steps)
        md, ms = statistics.median(times["deterministic"]), statistics.median(times["stochastic"])
        print(f"{prec:>5}: 4096-ray training step  deterministic {md:7.3f} ms   stochastic {ms:7.3f} ms   "
              f"({100.0 * (ms / md - 1.0):+.1f} %; min {min(times['deterministic']):.3f} / {min(times['stochastic']):.3f})")


if __name__ == "__main__":
    main()
