#!/usr/bin/env python3
"""Interleaved timing of one training step, unmasked vs fast_sampling (the ESS / ERT masked fine pass on compacted points).

    python tools/ab_masked_train.py [f32|f32x ...]

Per precision, scene (trained checkpoint, sharp family) and weights_threshold (0.25, 0.02): one Renderer in each mode on the
same network, 4096 pinhole rays, train_step (render under autograd, MSE, backward, FusedAdam) alternated between the two modes
for AB_ROUNDS rounds (default 12) of AB_STEPS steps (default 3), HIP events around each round.  Prints one JSON line per
configuration: median and min / max (the spread between repeats) ms per step of both modes, the share M / (192 n) of the
merged samples the fine network evaluated, and the live fine tiles of both modes (of 192 n / 32 unmasked tiles; the masked
step's are compact tiles, of ceil(M / 32) occupied ones).  Developer tool."""
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


def main():
    import nerf_replication_amd as pkg
    from nerf_replication_amd.training import FusedAdam, train_step
    precs = sys.argv[1:] or ["f32", "f32x"]
    rounds, steps = int(os.environ.get("AB_ROUNDS", "12")), int(os.environ.get("AB_STEPS", "3"))
    dev = torch.device("cuda:0")
    golden = os.path.join(REPO, "tests", "golden")
    base = torch.load(os.path.join(golden, "synthetic_ckpt.pth"), weights_only=True)["net"]
    base = {k: base[k] for k in orc.state_dict_keys()}
    trained = torch.load(os.path.join(golden, "trained_ckpt.pth"), weights_only=True)["net"]
    scenes = {"trained": {k: trained[k] for k in orc.state_dict_keys()}, "sharp": orc.weight_family(base, "sharp")}
    ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(1))[:N_RAYS]
    o, d = orc.pinhole_rays(800, 800, orc.camera_pose(40.0), pixel_ids=ids)
    o, d = o.to(dev).contiguous(), d.to(dev).contiguous()
    for prec in precs:
        for scene, sd in scenes.items():
            for thr in (0.25, 0.02):
                net = pkg.Network()
                net.load_state_dict(sd)
                net = net.to(dev).train()
                net.precision = prec
                with torch.no_grad():
                    target, _ = pkg.Renderer(net).render({"rays_o": o[None], "rays_d": d[None]})
                plain = pkg.Renderer(net)
                masked = pkg.Renderer(net)
                masked.fast_sampling, masked.weights_threshold = True, thr
                opt = FusedAdam(net.parameters(), lr=1e-6)       # tiny steps: the scene stays put over the measurement
                times = {"unmasked": [], "masked": []}
                pair = (("unmasked", plain), ("masked", masked))
                for rnd in range(rounds + 1):
                    for name, ren in pair if rnd % 2 == 0 else pair[::-1]:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(steps):
                            train_step(ren, opt, o, d, target)
                        e1.record()
                        torch.cuda.synchronize()
                        if rnd:
                            times[name].append(e0.elapsed_time(e1) / steps)
                # one more step of each with the statistics on (they clone device counters: kept out of the timed steps)
                plain.live_tile_stats, masked.live_tile_stats, masked.masked_stats = [], [], []
                train_step(plain, opt, o, d, target)
                train_step(masked, opt, o, d, target)
                torch.cuda.synchronize()
                m = int(masked.masked_stats[0][0].item())
                row = {"precision": prec, "scene": scene, "weights_threshold": thr, "n_rays": N_RAYS}
                for name in times:
                    t = times[name]
                    row[name + "_ms"] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
                row["masked_over_unmasked"] = round(statistics.median(times["masked"]) / statistics.median(times["unmasked"]), 4)
                row["points_evaluated_share"] = round(m / (192.0 * N_RAYS), 4)
                row["live_fine_tiles_unmasked"] = [int(plain.live_tile_stats[0][0].item()), plain.live_tile_stats[0][1]]
                row["live_fine_tiles_masked"] = [int(masked.live_tile_stats[0][0].item()), (m + 31) // 32]
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
