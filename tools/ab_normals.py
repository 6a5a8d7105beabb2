#!/usr/bin/env python3
"""Timing of the geometry pass: Renderer.render() and Renderer.render_geometry() alternating on the
800 x 800 oracle frame of the trained checkpoint, f32 and f32x, in one process; device events around each call after a warm-up
round; median and min-max per call, their ratio, and the bytes the pass's saved / gradient rows move per point.  Also checks that
the two calls agree on rgb and depth.  Writes profiles/normals_timing.json.  Needs an MI355X and the built library.

    python tools/ab_normals.py [--res 800] [--rounds 5] [--block-rays 4096] [--out profiles/normals_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import nerf_replication_amd as nerf  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-rays", type=int, default=4096)
    ap.add_argument("--angle", type=float, default=40.0)
    ap.add_argument("--precisions", default="f32,f32x")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "normals_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ab_normals.py needs a GPU"
    import nerf_oracle
    lib = nerf._lib.load()
    ck = torch.load(os.path.join(REPO, "tests", "golden", "trained_ckpt.pth"), weights_only=True)["net"]
    sd = {k: ck[k] for k in nerf_oracle.state_dict_keys()}
    o, d = nerf.generate_rays(nerf_oracle.camera_pose(args.angle), args.res, args.res, nerf_oracle.LEGO_CAMERA_ANGLE_X, "cuda")
    batch = {"rays_o": o[None], "rays_d": d[None]}
    n = o.shape[0]
    point_bytes = int(lib.nerf_density_gradient_point_bytes())
    rows = {"saved_rows_and_sign_bits": 4 * int(lib.nerf_train_save_floats(32)) // 32, "gradient_rows": 4 * int(lib.nerf_train_grad_floats(32)) // 32}
    rec = {"device": torch.cuda.get_device_name(0), "frame": [args.res, args.res], "pose_deg": args.angle, "rounds": args.rounds,
           "scene": "trained", "geometry_block_rays": args.block_rays, "workspace_bytes_per_point": point_bytes,
           "hbm_bytes_written_per_evaluated_point": rows, "sign_bit_bytes_per_point": 288,
           "timer": "device events around each call, render and render_geometry alternating in one process, one warm-up round", "runs": {}}
    for precision in args.precisions.split(","):
        net = nerf.Network()
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval()
        net.requires_grad_(False)
        net.precision = precision
        ren = nerf.Renderer(net)
        ren.geometry_block_rays = args.block_rays
        times = {"render": [], "render_geometry": []}
        with torch.no_grad():
            for rnd in range(args.rounds + 1):
                (rgb, depth), ms_r = event_ms(lambda: ren.render(batch))
                geo, ms_g = event_ms(lambda: ren.render_geometry(batch))
                if rnd == 0:
                    assert torch.equal(geo["rgb"], rgb) and torch.equal(geo["depth"], depth)
                    live = float((geo["acc"] > 0.5).float().mean())
                else:
                    times["render"].append(ms_r)
                    times["render_geometry"].append(ms_g)
        run = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for k, v in times.items()}
        run["geometry_over_render"] = run["render_geometry"]["median"] / run["render"]["median"]
        run["rays_per_s"] = {k: n / (run[k]["median"] * 1e-3) for k in times}
        run["share_of_rays_with_acc_above_half"] = live
        rec["runs"][precision] = run
        print(precision, json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
