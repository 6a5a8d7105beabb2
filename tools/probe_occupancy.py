#!/usr/bin/env python3
"""CPU probe for choosing the resolution and the dilation of an occupancy grid, no GPU needed: the oracle
(fp32, the reference's arithmetic) evaluates both models on the grid and renders pinhole rays; the NumPy restatement
tests/occupancy_reference.py builds the bitfields and looks the samples up.  Per (N, dilate) it prints the share of coarse / fine
samples culled, how many culled samples have sigma > 0 (what the cull would get wrong) and how many rays have one.

    python tools/probe_occupancy.py --scene trained --n 64 128 --dilate 0 1 [--rays 512] [--ckpt PATH]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import nerf_oracle  # noqa: E402
import occupancy_reference as O  # noqa: E402
from nerf_replication_amd.mesh import grid_axes  # noqa: E402


def state_dict(scene, ckpt):
    keys = nerf_oracle.state_dict_keys()
    if ckpt:
        ck = torch.load(ckpt, weights_only=True)
        ck = ck.get("net", ck)
        return {k: ck[k] for k in keys}
    if scene == "trained":
        ck = torch.load(os.path.join(REPO, "tests", "golden", "trained_ckpt.pth"), weights_only=True)["net"]
        return {k: ck[k] for k in keys}
    ck = torch.load(os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"), weights_only=True)["net"]
    return nerf_oracle.weight_family({k: ck[k] for k in keys}, scene)


def sigma_grid(sd, bbox, n, model):
    """Pre-ReLU sigma of one model on the grid points (fp32 coordinates of mesh.grid_axes): float32 [n, n, n]."""
    axes, _, _ = grid_axes(bbox, n)
    x, y, z = (torch.from_numpy(a.astype(np.float32)) for a in axes)
    out = torch.empty(n, n, n)
    view = torch.tensor([[0.0, 0.0, 1.0]])                       # sigma does not depend on the view direction
    for i in range(n):
        pts = torch.stack(torch.meshgrid(x[i:i + 1], y, z, indexing="ij"), dim=-1).reshape(1, n * n, 3)
        out[i] = nerf_oracle.network_forward(sd, pts, view, model)[0, :, 3].reshape(n, n)
    return out.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="trained", help='"trained" or a weight family of the oracle (base, sharp, white)')
    ap.add_argument("--ckpt", default=None, help="a checkpoint of your own instead of --scene")
    ap.add_argument("--n", type=int, nargs="+", default=[64])
    ap.add_argument("--dilate", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--level", type=float, default=0.0)
    ap.add_argument("--box", type=float, default=2.0, help="half edge of the cube around the origin")
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--angle", type=float, default=40.0)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd = state_dict(args.scene, args.ckpt)
    bbox = [-args.box] * 3 + [args.box] * 3
    ids = torch.from_numpy(np.random.default_rng(args.seed).choice(800 * 800, args.rays, replace=False))
    o, d = nerf_oracle.pinhole_rays(800, 800, nerf_oracle.camera_pose(args.angle), pixel_ids=ids)
    with torch.no_grad():
        _, _, parts = nerf_oracle.render(sd, o[None], d[None], return_parts=True)
    t_c, sig_c = parts["t_coarse"].numpy(), parts["raw_coarse"][..., 3].numpy()
    t_f, sig_f = parts["t_sorted"].numpy(), parts["raw_fine"][..., 3].numpy()
    o, d = o.numpy(), d.numpy()
    print(f"scene {args.ckpt or args.scene}: {args.rays} rays, pose {args.angle} deg, bbox +-{args.box}, level {args.level}")
    print("| N | dil | culled coarse / fine samples | samples culled with sigma > 0 (c / f) | rays with such a sample |")
    print("|---|---|---|---|---|")
    for n in args.n:
        with torch.no_grad():
            fields = {m: sigma_grid(sd, bbox, n, m) for m in ("", "fine")}
        dims = (n, n, n)
        lo, inv = O.lookup_frame(bbox, dims)
        for dil in args.dilate:
            keep_c = O.keep(o, d, t_c, O.build(fields[""], args.level, dil), dims, lo, inv)
            keep_f = O.keep(o, d, t_f, O.build(fields["fine"], args.level, dil), dims, lo, inv)
            bad_c, bad_f = ~keep_c & (sig_c > 0), ~keep_f & (sig_f > 0)
            print(f"| {n} | {dil} | {1 - keep_c.mean():.3f} / {1 - keep_f.mean():.3f} | {bad_c.sum()} / {bad_f.sum()} | "
                  f"{(bad_c.any(1) | bad_f.any(1)).sum()} / {args.rays} |", flush=True)


if __name__ == "__main__":
    main()
