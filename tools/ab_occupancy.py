#!/usr/bin/env python3
"""A/B of the occupancy grid on the 800 x 800 frame: plain render, occupancy (N = 128, dilate 1),
fast_sampling at the reference's threshold 0.25, and both, on the trained checkpoint and the "sharp" family, in f32 and f32x.
The variants alternate in one process; device events around Renderer.render after a warm-up round; median and min-max per
variant, the share of points evaluated, the PSNR against the plain HIP render of the same process, and the grid build time.
Writes profiles/occupancy_timing.json.  Needs an MI355X and the built library.

    python tools/ab_occupancy.py [--res 800] [--rounds 7] [--n 128] [--dilate 1] [--out profiles/occupancy_timing.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import nerf_replication_amd as nerf  # noqa: E402

BOX = [-2.0, -2.0, -2.0, 2.0, 2.0, 2.0]
VARIANTS = (("plain", False, False), ("occupancy", True, False), ("fast_sampling", False, True), ("both", True, True))


def state_dict(scene):
    import nerf_oracle
    keys = nerf_oracle.state_dict_keys()
    if scene == "trained":
        ck = torch.load(os.path.join(REPO, "tests", "golden", "trained_ckpt.pth"), weights_only=True)["net"]
        return {k: ck[k] for k in keys}
    ck = torch.load(os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"), weights_only=True)["net"]
    return nerf_oracle.weight_family({k: ck[k] for k in keys}, scene)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def psnr(a, b):
    mse = ((a.double() - b.double()) ** 2).mean().item()
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--angle", type=float, default=40.0)
    ap.add_argument("--scenes", default="trained,sharp")
    ap.add_argument("--precisions", default="f32,f32x")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ab_occupancy.py needs a GPU"
    import nerf_oracle
    o, d = nerf.generate_rays(nerf_oracle.camera_pose(args.angle), args.res, args.res, nerf_oracle.LEGO_CAMERA_ANGLE_X, "cuda")
    batch = {"rays_o": o[None], "rays_d": d[None]}
    n = o.shape[0]
    ones = torch.ones(2, 2, 2, device="cuda")
    rec = {"device": torch.cuda.get_device_name(0), "frame": [args.res, args.res], "pose_deg": args.angle, "rounds": args.rounds,
           "grid": {"N": args.n, "dilate": args.dilate, "bbox": BOX, "level": 0.0}, "weights_threshold": 0.25,
           "timer": "device events around Renderer.render, variants alternating in one process, one warm-up round", "runs": {}}
    for scene in args.scenes.split(","):
        for precision in args.precisions.split(","):
            net = nerf.Network()
            net.load_state_dict(state_dict(scene), strict=True)
            net = net.cuda().eval()
            net.precision = precision
            with torch.no_grad():
                nerf.OccupancyGrid.from_network(net, BOX, args.n, dilate=args.dilate)               # warm-up: packing, code objects
                builds = [event_ms(lambda: nerf.OccupancyGrid.from_network(net, BOX, args.n, dilate=args.dilate)) for _ in range(3)]
            grid = builds[-1][0]
            renderers = {}
            for name, occ, fast in VARIANTS:
                r = renderers[name] = nerf.Renderer(net)
                r.fast_sampling, r.weights_threshold = fast, 0.25
                if occ:
                    r.occupancy, r.occupancy_stats = grid, []
            times = {name: [] for name in renderers}
            images = {}
            with torch.no_grad():
                for rnd in range(args.rounds + 1):
                    for name, r in renderers.items():
                        (rgb, _), ms = event_ms(lambda: r.render(batch))
                        if rnd == 0:
                            images[name] = rgb.clone()
                        else:
                            times[name].append(ms)
            run = {"grid_build_ms": {"median": statistics.median(b[1] for b in builds), "all": [b[1] for b in builds]},
                   "occupied_fraction": {"coarse": grid.occupied_fraction(""), "fine": grid.occupied_fraction("fine")}, "variants": {}}
            plain = statistics.median(times["plain"])
            for name, r in renderers.items():
                ts = times[name]
                v = {"ms": {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "all": ts},
                     "rays_per_s": n / (statistics.median(ts) * 1e-3), "speedup_vs_plain": plain / statistics.median(ts),
                     "psnr_vs_plain_db": psnr(images[name], images["plain"]),
                     "rays_differing_from_plain": int((images[name] != images["plain"]).any(dim=1).sum())}
                # the points evaluated: the variants without a grid are counted once, outside the timing, through a grid that culls nothing
                stats = r.occupancy_stats
                if stats is None:
                    counter = nerf.Renderer(net)
                    counter.fast_sampling, counter.weights_threshold = r.fast_sampling, r.weights_threshold
                    counter.occupancy, counter.occupancy_stats = nerf.OccupancyGrid.from_fields([-8.0] * 3 + [8.0] * 3, coarse=ones, fine=ones), []
                    with torch.no_grad():
                        counter.render(batch)
                    stats = counter.occupancy_stats
                ev, total = stats[-1]
                ev = ev.tolist()
                v["points_evaluated_share"] = {"coarse": ev[0] / total[0], "fine": ev[1] / total[1], "all": (ev[0] + ev[1]) / sum(total)}
                run["variants"][name] = v
            rec["runs"][f"{scene}/{precision}"] = run
            print(scene, precision, json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
