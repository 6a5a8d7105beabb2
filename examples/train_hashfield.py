#!/usr/bin/env python3
"""Train a hash-grid radiance field (HashField + HashRenderer + FusedAdam) against images rendered from a teacher checkpoint: the
teacher setup of examples/train_synthetic.py (renders of tests/golden/synthetic_ckpt.pth from a ring of poses, one view held out),
4096 random rays per step, MSE on the rendered RGB.

    python examples/train_hashfield.py --steps 600
    python examples/train_hashfield.py --steps 600 --occupancy 64 --refresh-every 16      # cull empty space while training
    python examples/train_hashfield.py --steps 600 --n-samples 64 --importance 64 --perturb   # resample from the field's own density

--occupancy N rebuilds an N^3 occupancy grid from the field itself (HashField.occupancy_grid) every --refresh-every steps; a grid made
from fields carries no staleness key, so this loop owns the schedule; the first --occupancy-from steps run unculled.  Prints ms per
step and the held-out PSNR.  --n-samples Sc --importance Sf renders every ray on Sc coarse depths plus Sf depths drawn from the weights
of a density-only coarse pass (HashRenderer.N_importance); --perturb jitters the coarse depths inside their strata and draws random u
while training (the held-out evaluation renders with perturb off).  --deterministic-table sums the hash table's gradient exactly and order-independently
(HashEncoder(deterministic=True)); the two networks' weight and bias gradients then keep their fp32 atomics.  --deterministic turns
on the table and both networks together (HashField(deterministic=True)): every sum of the step is exact and order-independent, and
two runs from one seed end with the same parameters, byte for byte -- the last line printed is then a digest of them.
"""
import argparse
import hashlib
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
    ap.add_argument("--views", type=int, default=64,
                    help="training views on the ring (train_synthetic.py uses 16: enough for the MLP's smooth prior, while a hash grid "
                         "fits 16 views to 45 dB and the held-out one to 15)")
    ap.add_argument("--res", type=int, default=200)
    ap.add_argument("--samples", "--n-samples", dest="samples", type=int, default=192,
                    help="depths per ray (HashRenderer.N_samples, 1..192); with --importance the coarse count")
    ap.add_argument("--importance", type=int, default=0, metavar="SF",
                    help="fine depths per ray, resampled from the coarse pass's weights (HashRenderer.N_importance; "
                         "--n-samples + SF <= 192)")
    ap.add_argument("--perturb", action="store_true",
                    help="train on jittered coarse depths and random u (HashRenderer.perturb); evaluation stays deterministic")
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--log2-hashmap-size", type=int, default=19)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--half-extent", type=float, default=2.0, metavar="R", help="the field's box is [-R, R]^3")
    ap.add_argument("--occupancy", type=int, default=0, metavar="N", help="cull with an occupancy grid of N^3 points over the box")
    ap.add_argument("--refresh-every", type=int, default=16, metavar="K", help="rebuild the grid from the field every K steps")
    ap.add_argument("--occupancy-from", type=int, default=100, metavar="STEP",
                    help="first step that is culled: a fresh field has no density to speak of, and a grid built from it would cull "
                         "every sample (no sample, no gradient)")
    ap.add_argument("--out", default=None, help="write the trained field's state dict here")
    ap.add_argument("--deterministic-table", action="store_true",
                    help="sum the hash table's gradient exactly, in an order-independent way (HashEncoder(deterministic=True))")
    ap.add_argument("--deterministic", action="store_true",
                    help="exact, order-independent sums for the table and for both networks' weight and bias gradients "
                         "(HashField(deterministic=True))")
    args = ap.parse_args()
    if args.occupancy and args.occupancy < 2:
        ap.error("--occupancy needs at least 2 grid points per axis")
    if args.refresh_every < 1:
        ap.error("--refresh-every must be at least 1")
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
    encoder = nerf.HashEncoder(input_dim=3, num_levels=args.levels, level_dim=2, base_resolution=16,
                               log2_hashmap_size=args.log2_hashmap_size, desired_resolution=2048,
                               deterministic=args.deterministic_table or args.deterministic)
    half = float(args.half_extent)
    field = nerf.HashField((-half, -half, -half, half, half, half), encoder=encoder, deterministic=args.deterministic).cuda()
    ren = nerf.HashRenderer(field)                             # the held-out evaluation: never culled
    ren.N_samples, ren.N_importance = args.samples, args.importance
    train_ren = nerf.HashRenderer(field)
    train_ren.N_samples, train_ren.N_importance, train_ren.perturb = args.samples, args.importance, args.perturb
    if args.occupancy:
        train_ren.stats = []
    opt = FusedAdam(field.parameters(), lr=args.lr, eps=1e-15, clip_value=40.0)
    gen = torch.Generator(device=dev).manual_seed(1)

    def held_out_psnr():
        with torch.no_grad():
            rgb, _ = ren.render({"rays_o": test[0][None], "rays_d": test[1][None]})
        return -10.0 * math.log10(torch.mean((rgb - test[2]) ** 2).item())

    print("step     loss    held-out PSNR   ms/step   seconds")
    start = time.perf_counter()
    t0, last, refreshes = start, 0, 0
    for step in range(args.steps + 1):
        if step % 100 == 0 or step == args.steps:
            torch.cuda.synchronize()
            now = time.perf_counter()
            dt = (now - t0) / max(1, step - last) * 1e3
            print("{:5d}  {:9.6f}   {:6.2f} dB      {:6.1f}   {:7.2f}".format(step, float("nan") if step == 0 else loss.item(),
                                                                           held_out_psnr(), dt, now - start), flush=True)
            t0, last = time.perf_counter(), step
        if step == args.steps:
            break
        if args.occupancy and step >= args.occupancy_from and (step - args.occupancy_from) % args.refresh_every == 0:
            train_ren.occupancy = field.occupancy_grid(N=args.occupancy, level=0.0, dilate=1)
            refreshes += 1
        ids = torch.randint(0, O.shape[0], (4096,), device=dev, generator=gen)
        loss = train_step(train_ren, opt, O[ids].contiguous(), D[ids].contiguous(), C[ids].contiguous())
    if args.occupancy and train_ren.stats:
        evaluated, total = sum(m for m, _ in train_ren.stats), sum(p for _, p in train_ren.stats)
        print("occupancy grid {0}^3, rebuilt every {1} steps ({2} builds): the field evaluated {3:.3f} of the samples"
              .format(args.occupancy, args.refresh_every, refreshes, evaluated / total))
    print("held-out PSNR after {0} steps: {1:.2f} dB".format(args.steps, held_out_psnr()))
    if args.out:
        torch.save(field.state_dict(), args.out)
        print("saved", args.out)
    if args.deterministic:
        digest = hashlib.sha256()
        for p in field.parameters():
            digest.update(p.detach().cpu().numpy().tobytes())
        print("parameters sha256:", digest.hexdigest())


if __name__ == "__main__":
    main()
