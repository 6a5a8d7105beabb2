#!/usr/bin/env python3
"""Times density_grid and isosurface on the trained checkpoint (device events, median of repeated runs after a warm-up) and
writes profiles/mesh_timing.json.  Needs an MI355X and the built library.

    python tools/time_mesh.py [--n 256] [--reps 7] [--out profiles/mesh_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import nerf_replication_amd as nerf  # noqa: E402
from nerf_replication_amd.mesh import grid_axes  # noqa: E402

FLOP_PER_POINT = 982528          # density-only network (include/nerf_mi355x.h, nerf_mlp_forward_rays_density)


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=os.path.join(REPO, "tests", "golden", "trained_ckpt.pth"))
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--box", type=float, default=1.5, help="half edge of the cube around the origin")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_mesh.py needs a GPU"
    box = [-args.box] * 3 + [args.box] * 3
    _, origin, step = grid_axes(box, args.n)
    net = nerf.Network()
    nerf.load_network(net, args.ckpt)
    net = net.cuda().eval()
    rec = {"device": torch.cuda.get_device_name(0), "N": args.n, "bbox": box, "reps": args.reps, "checkpoint": os.path.basename(args.ckpt),
           "timer": "device events around the call; isosurface includes its one host read of the two counts", "precisions": {}}
    for precision in ("f32", "f16"):
        net.precision = precision
        grid = nerf.density_grid(net, box, args.n)                       # warm-up: weight packing, code objects
        level = 0.5 * (grid.median().item() + grid.max().item())
        nerf.isosurface(grid, level, origin, step)
        grid, ms_grid = timed(lambda: nerf.density_grid(net, box, args.n), args.reps)
        (v, t), ms_iso = timed(lambda: nerf.isosurface(grid, level, origin, step), args.reps)
        med_grid, med_iso = statistics.median(ms_grid), statistics.median(ms_iso)
        rec["precisions"][precision] = {
            "level": level, "V": int(v.shape[0]), "T": int(t.shape[0]),
            "density_grid_ms": {"median": med_grid, "min": min(ms_grid), "max": max(ms_grid), "all": ms_grid},
            "density_grid_tflops": args.n ** 3 * FLOP_PER_POINT / (med_grid * 1e-3) / 1e12,
            "isosurface_ms": {"median": med_iso, "min": min(ms_iso), "max": max(ms_iso), "all": ms_iso},
        }
        print(precision, json.dumps(rec["precisions"][precision]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
