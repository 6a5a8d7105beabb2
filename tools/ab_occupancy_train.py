#!/usr/bin/env python3
"""Interleaved timing of one training step: plain, culled by an occupancy grid (Renderer.train_occupancy), masked by fast_sampling,
and the grid's refresh.

    python tools/ab_occupancy_train.py [f32|f32x ...] [--rounds 10] [--steps 3] [--n 128] [--dilate 1] [--hold 2] [--out FILE]

Per precision and scene (trained checkpoint, sharp family): one network, 4096 pinhole rays, a grid of N^3 points on [-2,2]^3, and
four variants alternated in one process for `rounds` rounds (one more comes first and is not counted), HIP events around each:
  a  `steps` plain train_steps (render under autograd, MSE, backward, FusedAdam)
  b  `steps` culled train_steps, no refresh inside the window (train_occupancy_every is out of reach)
  c  `steps` masked train_steps (fast_sampling, weights_threshold 0.25)
  d  one OccupancyGrid.refresh of the fine model alone
Prints one JSON line per configuration and writes them all to profiles/occupancy_train_timing.json: median and min / max ms of every
variant, b / a, (b + d / 16) / a (the step with its refresh amortised over the default train_occupancy_every), c / a, the share of
the merged samples the fine network evaluated in b and in c, and the live fine tiles.  Needs an MI355X and the built library: without
a GPU it fails, it does not fall back.  Developer tool."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import nerf_oracle as orc  # noqa: E402  (pinhole rays, weight families)

N_RAYS = 4096
BOX = [-2.0, -2.0, -2.0, 2.0, 2.0, 2.0]
EVERY = 16                  # Renderer.train_occupancy_every's default: what d is amortised over


def _summary(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def main():
    import nerf_replication_amd as pkg
    from nerf_replication_amd.training import FusedAdam, train_step
    ap = argparse.ArgumentParser()
    ap.add_argument("precisions", nargs="*", default=["f32", "f32x"])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--hold", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_train_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_occupancy_train.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    golden = os.path.join(REPO, "tests", "golden")
    base = torch.load(os.path.join(golden, "synthetic_ckpt.pth"), weights_only=True)["net"]
    base = {k: base[k] for k in orc.state_dict_keys()}
    trained = torch.load(os.path.join(golden, "trained_ckpt.pth"), weights_only=True)["net"]
    scenes = {"trained": {k: trained[k] for k in orc.state_dict_keys()}, "sharp": orc.weight_family(base, "sharp")}
    ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(1))[:N_RAYS]
    o, d = orc.pinhole_rays(800, 800, orc.camera_pose(40.0), pixel_ids=ids)
    o, d = o.to(dev).contiguous(), d.to(dev).contiguous()
    rows = []
    for prec in args.precisions:
        for scene, sd in scenes.items():
            net = pkg.Network()
            net.load_state_dict(sd)
            net = net.to(dev).train()
            net.precision = prec
            with torch.no_grad():
                target, _ = pkg.Renderer(net).render({"rays_o": o[None], "rays_d": d[None]})
            grid = pkg.OccupancyGrid.from_network(net, BOX, args.n, dilate=args.dilate, models=("fine",))
            grid.hold = args.hold
            plain, culled, masked = pkg.Renderer(net), pkg.Renderer(net), pkg.Renderer(net)
            culled.train_occupancy, culled.train_occupancy_every = grid, 1 << 60      # the refresh is variant d, never inside b
            masked.fast_sampling, masked.weights_threshold = True, 0.25
            opt = FusedAdam(net.parameters(), lr=1e-6)       # tiny steps: the scene stays put over the measurement

            def run(name):
                if name == "refresh":
                    grid.refresh(net, models=("fine",))
                    return 1
                ren = {"plain": plain, "culled": culled, "masked": masked}[name]
                for _ in range(args.steps):
                    train_step(ren, opt, o, d, target)
                return args.steps

            order = ("plain", "culled", "masked", "refresh")
            times = {name: [] for name in order}
            for rnd in range(args.rounds + 1):
                for name in order if rnd % 2 == 0 else order[::-1]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    per = run(name)
                    e1.record()
                    torch.cuda.synchronize()
                    if rnd:
                        times[name].append(e0.elapsed_time(e1) / per)
            # one more step of each with the statistics on (they clone device counters: kept out of the timed steps)
            for ren in (plain, culled, masked):
                ren.live_tile_stats, ren.masked_stats = [], []
                train_step(ren, opt, o, d, target)
            torch.cuda.synchronize()
            m_b, m_c = int(culled.masked_stats[0][0].item()), int(masked.masked_stats[0][0].item())
            a, b, c, r = (statistics.median(times[k]) for k in order)
            row = {"precision": prec, "scene": scene, "n_rays": N_RAYS, "grid": {"N": args.n, "dilate": args.dilate, "hold": args.hold, "bbox": BOX},
                   "rounds": args.rounds, "steps_per_round": args.steps,
                   "a_plain_ms": _summary(times["plain"]), "b_culled_ms": _summary(times["culled"]),
                   "c_masked_025_ms": _summary(times["masked"]), "d_refresh_fine_ms": _summary(times["refresh"]),
                   "b_over_a": round(b / a, 4), "b_plus_d16_over_a": round((b + r / EVERY) / a, 4), "c_over_a": round(c / a, 4),
                   "points_evaluated_share_culled": round(m_b / (192.0 * N_RAYS), 4),
                   "points_evaluated_share_masked": round(m_c / (192.0 * N_RAYS), 4),
                   "occupied_fraction_fine": round(grid.occupied_fraction("fine"), 4),
                   "live_fine_tiles_plain": [int(plain.live_tile_stats[0][0].item()), plain.live_tile_stats[0][1]],
                   "live_fine_tiles_culled": [int(culled.live_tile_stats[0][0].item()), (m_b + 31) // 32],
                   "live_fine_tiles_masked": [int(masked.live_tile_stats[0][0].item()), (m_c + 31) // 32]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
