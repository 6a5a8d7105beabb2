#!/usr/bin/env python3
"""Interleaved timing of the ray-gradient paths against the plain training step (4096 rays, trained checkpoint).

    python tools/ab_ray_grad.py [f32|f32x ...] [--json PATH]

Per precision, three steps on the same rays, alternated for AB_ROUNDS rounds (default 30) of AB_STEPS steps (default 5), HIP
events around each round, medians per step:
  (a) plain   train() step: render under autograd, MSE, backward, FusedAdam (tools/ab_stochastic_train.py's step);
  (b) rays    the same step with rays_o / rays_d requiring grad (the rays get their gradient too);
  (c) frozen  pose step of a frozen network (eval(), requires_grad_(False)): render, MSE, backward to the rays only.
--json PATH also writes the figures as JSON.  Developer tool; the figures are recorded in DESIGN.md section 2.5.1 and
profiles/ray_grad_timing.json."""
import argparse
import json
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
    from nerf_replication_amd.training import FusedAdam
    ap = argparse.ArgumentParser()
    ap.add_argument("precisions", nargs="*", help="f32 and / or f32x (default: both)")
    ap.add_argument("--json", default=None, help="also write the figures to this JSON file")
    args = ap.parse_args()
    precs = args.precisions or ["f32", "f32x"]
    for p in precs:
        if p not in ("f32", "f32x"):
            ap.error(f"precision {p!r}: the ray gradients are built for f32 and f32x")
    rounds, steps = int(os.environ.get("AB_ROUNDS", "30")), int(os.environ.get("AB_STEPS", "5"))
    dev = torch.device("cuda:0")
    ck = torch.load(os.path.join(REPO, "tests", "golden", "trained_ckpt.pth"), weights_only=True)["net"]
    sd = {k: ck[k] for k in orc.state_dict_keys()}
    ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(1))[:4096]
    o, d = orc.pinhole_rays(800, 800, orc.camera_pose(30.0), pixel_ids=ids)
    o, d = o.to(dev).contiguous(), d.to(dev).contiguous()
    o2, d2 = orc.pinhole_rays(800, 800, orc.camera_pose(32.0), pixel_ids=ids)
    o2, d2 = o2.to(dev).contiguous(), d2.to(dev).contiguous()
    result = {}
    for prec in precs:
        net = pkg.Network(); net.load_state_dict(sd); net = net.to(dev).train(); net.precision = prec
        frozen = pkg.Network(); frozen.load_state_dict(sd); frozen = frozen.to(dev).eval().requires_grad_(False)
        frozen.precision = prec
        with torch.no_grad():                            # the view from a camera 2 degrees away: a live gradient everywhere
            target, _ = pkg.Renderer(frozen).render({"rays_o": o2[None], "rays_d": d2[None]})
        ren, fren = pkg.Renderer(net), pkg.Renderer(frozen)
        opt = FusedAdam(net.parameters(), lr=1e-6)       # tiny steps: the scene stays put over the measurement
        og, dg = o.clone().requires_grad_(True), d.clone().requires_grad_(True)

        def train(rays_grad):
            opt.zero_grad(set_to_none=True)
            og.grad = dg.grad = None
            ro, rd = (og, dg) if rays_grad else (o, d)
            rgb, _ = ren.render({"rays_o": ro[None], "rays_d": rd[None]})
            torch.nn.functional.mse_loss(rgb, target).backward()
            opt.step()

        def pose():
            og.grad = dg.grad = None
            rgb, _ = fren.render({"rays_o": og[None], "rays_d": dg[None]})
            torch.nn.functional.mse_loss(rgb, target).backward()

        modes = [("plain", lambda: train(False)), ("rays", lambda: train(True)), ("frozen", pose)]
        times = {k: [] for k, _ in modes}
        for rnd in range(rounds + 1):
            order = modes[rnd % 3:] + modes[:rnd % 3]
            for name, fn in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(e0.elapsed_time(e1) / steps)
        med = {k: statistics.median(v) for k, v in times.items()}
        result[prec] = {"median_ms": med, "min_ms": {k: min(v) for k, v in times.items()},
                        "rays_over_plain": med["rays"] / med["plain"], "frozen_over_plain": med["frozen"] / med["plain"],
                        "rounds": rounds, "steps_per_round": steps}
        print(f"{prec:>5}: 4096 rays  (a) plain {med['plain']:7.3f} ms   (b) rays {med['rays']:7.3f} ms "
              f"({med['rays'] / med['plain']:.3f}x)   (c) frozen pose step {med['frozen']:7.3f} ms ({med['frozen'] / med['plain']:.3f}x)")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
