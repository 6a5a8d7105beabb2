#!/usr/bin/env python3
"""Train a freshly initialised network against images rendered from a teacher checkpoint: the reference's
training step (trainers/nerf.py:27-33 + trainer.py:53-60: 4096 random rays, MSE on the fine RGB, clip 40,
Adam 5e-4, exponential decay) on the HIP training path, with periodic checkpoints in the reference's layout.

    python examples/train_synthetic.py --steps 600 --precision f32x --out /tmp/nerf_train
    python examples/train_synthetic.py --steps 600 --occupancy 64          # cull the fine pass with an occupancy grid

There is no dataset offline, so the "photos" are renders of tests/golden/synthetic_ckpt.pth from random poses."""
import argparse
import math
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "examples"))
import nerf_replication_amd as nerf  # noqa: E402
from nerf_replication_amd.training import FusedAdam, train_step  # noqa: E402
from render_frame import camera_pose  # noqa: E402

FOV = 0.6911112070083618


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher", default=os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"))
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--res", type=int, default=200)
    ap.add_argument("--precision", default="f32x", choices=["f32", "f32x"])
    ap.add_argument("--out", default="nerf_train")
    ap.add_argument("--perturb", action="store_true",
                    help="train with the reference's stochastic sampling (task: train): jittered coarse depths, random fine u")
    ap.add_argument("--fast-sampling", action="store_true",
                    help="train with the reference's ESS / ERT masked fine pass (fast_sampling): the fine network runs on, stores and "
                         "back-propagates the valid merged samples only; deterministic sampling (not with --perturb)")
    ap.add_argument("--weights-threshold", type=float, default=0.25,
                    help="ESS threshold on the coarse weights with --fast-sampling (reference default 0.25; 0.02 keeps far more fine samples)")
    ap.add_argument("--occupancy", type=int, default=0, metavar="N",
                    help="cull the fine pass of the training step with an occupancy grid of N^3 points on [-2,2]^3 (Renderer.train_occupancy), "
                         "rebuilt from the network as it trains; works with --perturb and with --fast-sampling")
    ap.add_argument("--occupancy-every", type=int, default=16, metavar="K", help="one grid build serves K steps (train_occupancy_every)")
    ap.add_argument("--occupancy-hold", type=int, default=1, metavar="H",
                    help="a grid point stays occupied for H refreshes after it was last above the level (OccupancyGrid.hold)")
    args = ap.parse_args()
    if args.fast_sampling and args.perturb:
        ap.error("--fast-sampling trains with deterministic sampling: leave --perturb out")
    if args.occupancy and args.occupancy < 2:
        ap.error("--occupancy needs at least 2 grid points per axis")
    dev = "cuda"

    teacher = nerf.Network(); nerf.load_network(teacher, args.teacher); teacher = teacher.cuda().eval()
    t_ren = nerf.Renderer(teacher)
    rays_o, rays_d, colors = [], [], []
    with torch.no_grad():
        for v in range(args.views + 1):                       # the last view is held out
            o, d = nerf.generate_rays(camera_pose(360.0 * v / (args.views + 1), elevation_deg=20.0 + 25.0 * (v % 3)),
                                      args.res, args.res, FOV, dev)
            rgb, _ = t_ren.render({"rays_o": o[None], "rays_d": d[None]})
            rays_o.append(o); rays_d.append(d); colors.append(rgb)
    test = (rays_o.pop(), rays_d.pop(), colors.pop())
    O, D, C = torch.cat(rays_o), torch.cat(rays_d), torch.cat(colors)

    torch.manual_seed(0)
    net = nerf.Network().cuda().train()                         # nn.Linear default init, as the reference
    net.precision = args.precision
    ren = nerf.Renderer(net)                                    # deterministic: the held-out evaluation
    train_ren = ren
    if args.perturb:
        train_ren = nerf.Renderer(net)
        train_ren.task, train_ren.perturb = "train", True
    if args.fast_sampling:
        train_ren = nerf.Renderer(net)
        train_ren.fast_sampling, train_ren.weights_threshold = True, args.weights_threshold
    refreshes = [0]
    if args.occupancy:
        if train_ren is ren:
            train_ren = nerf.Renderer(net)
        grid = nerf.OccupancyGrid.from_network(net, [-2.0, -2.0, -2.0, 2.0, 2.0, 2.0], args.occupancy, dilate=1, models=("fine",))
        grid.hold = args.occupancy_hold
        refresh = grid.refresh

        def counted(*a, **k):
            refreshes[0] += 1
            return refresh(*a, **k)
        grid.refresh = counted
        train_ren.train_occupancy, train_ren.train_occupancy_every = grid, args.occupancy_every
        train_ren.masked_stats = []
    opt = FusedAdam(net.parameters(), lr=5e-4, eps=1e-8, clip_value=40.0)
    lr0, gen = 5e-4, torch.Generator(device=dev).manual_seed(1)

    def held_out_psnr():
        net.eval()
        with torch.no_grad():
            rgb, _ = ren.render({"rays_o": test[0][None], "rays_d": test[1][None]})
        net.train()
        return -10.0 * math.log10(torch.mean((rgb - test[2]) ** 2).item())

    print("step     loss    held-out PSNR   ms/step")
    t0, last = time.perf_counter(), 0
    for step in range(args.steps + 1):
        if step % 100 == 0:
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / max(1, step - last) * 1e3
            print("{:5d}  {:9.6f}   {:6.2f} dB      {:6.1f}".format(step, float("nan") if step == 0 else loss.item(), held_out_psnr(), dt))
            t0, last = time.perf_counter(), step
        if step == args.steps:
            break
        ids = torch.randint(0, O.shape[0], (4096,), device=dev, generator=gen)
        opt.lr = FusedAdam.exponential_lr(lr0, epoch=step / 50.0)          # ExponentialLR, one "epoch" = 50 iterations here
        loss = train_step(train_ren, opt, O[ids].contiguous(), D[ids].contiguous(), C[ids].contiguous())
    if args.occupancy and train_ren.masked_stats:
        evaluated = sum(int(m.item()) for m, _ in train_ren.masked_stats)
        capacity = sum(cap for _, cap in train_ren.masked_stats)
        print("occupancy grid {0}^3, every {1}, hold {2}: the fine network evaluated {3:.3f} of the merged samples; {4} refreshes in {5} steps"
              .format(args.occupancy, args.occupancy_every, args.occupancy_hold, evaluated / capacity, refreshes[0], args.steps))
    nerf.save_model(net, opt, None, None, args.out, epoch=args.steps // 50, last=True)
    print("saved", os.path.join(args.out, "latest.pth"))


if __name__ == "__main__":
    main()
