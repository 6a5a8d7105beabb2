#!/usr/bin/env python3
"""Times density_grid, isosurface and the mesh clean-up (connected components, the keep-largest filter, vertex colours) on the
trained checkpoint (device events, median of repeated runs after a warm-up) and writes profiles/mesh_timing.json.  Needs an MI355X
and the built library.

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
from nerf_replication_amd.mesh import _Components, grid_axes  # noqa: E402

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


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


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
           "timer": "device events around the call; isosurface, components and filter each include their one host read of the counts",
           "precisions": {}}
    for precision in ("f32", "f16"):
        net.precision = precision
        grid = nerf.density_grid(net, box, args.n)                       # warm-up: weight packing, code objects
        level = 0.5 * (grid.median().item() + grid.max().item())
        nerf.isosurface(grid, level, origin, step)
        grid, ms_grid = timed(lambda: nerf.density_grid(net, box, args.n), args.reps)
        (v, t), ms_iso = timed(lambda: nerf.isosurface(grid, level, origin, step), args.reps)
        med_grid = statistics.median(ms_grid)
        # clean-up: the components of the whole surface, the filter that keeps the largest one, colours at its vertices
        comps = _Components(t, v.shape[0])                               # warm-up
        comps.filter(v, comps.select(None, 1))
        comps, ms_comp = timed(lambda: _Components(t, v.shape[0]), args.reps)
        (v1, t1, _), ms_filter = timed(lambda: comps.filter(v, comps.select(None, 1)), args.reps)
        ms_colors = None
        if precision == "f32":                                           # head-on colours need the normals: f32 / f32x
            nerf.vertex_colors(net, v1)
            _, ms_colors = timed(lambda: nerf.vertex_colors(net, v1), args.reps)
        rec["precisions"][precision] = {
            "level": level, "V": int(v.shape[0]), "T": int(t.shape[0]), "C": int(comps.table.label.shape[0]),
            "V_kept": int(v1.shape[0]), "T_kept": int(t1.shape[0]),
            "density_grid_ms": stats(ms_grid),
            "density_grid_tflops": args.n ** 3 * FLOP_PER_POINT / (med_grid * 1e-3) / 1e12,
            "isosurface_ms": stats(ms_iso),
            "components_ms": stats(ms_comp),
            "filter_keep_largest_1_ms": stats(ms_filter),
            "vertex_colors_ms": None if ms_colors is None else stats(ms_colors),
        }
        print(precision, json.dumps(rec["precisions"][precision]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
