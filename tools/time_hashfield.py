#!/usr/bin/env python3
"""Times the hash-grid radiance field (HashField + HashRenderer) against Renderer on the 8 x 256 MLP, in the same process on the same
GPU: an 800 x 800 frame at 192 samples per ray (the field without and with an occupancy grid; Renderer in f32 and f32x on
tests/golden/synthetic_ckpt.pth) and a 4096-ray training step (train_step with FusedAdam on each).  Device events around whole calls
(render() or train_step() to the last enqueued kernel, allocations and the culled path's host synchronisation included), a warm-up of
every case, then alternating rounds; the record keeps every sample and reports median with min-max: the method of
tools/time_fused_mlp.py.  The field is first trained for --train-steps steps against the teacher (the loop of
examples/train_hashfield.py), so that its occupancy grid culls what a trained field culls.  Then examples/train_hashfield.py and
examples/train_synthetic.py run as fresh processes and their held-out PSNR is recorded against wall-clock seconds.
Writes profiles/hashfield_timing.json.  Needs an MI355X and the built library.

    python tools/time_hashfield.py [--rounds 7] [--train-steps 300] [--example-steps 300] [--example-views 64] [--out profiles/hashfield_timing.json]

No speed is asserted: the two renderers draw different models (a 16-level hash grid with two small heads, 192 uniform samples; two
8 x 256 MLPs, 64 + 128 hierarchical samples), so the figures say what each costs, not that one replaces the other at equal quality.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "examples"))
import nerf_replication_amd as nerf  # noqa: E402
from nerf_replication_amd.training import FusedAdam, train_step  # noqa: E402
from render_frame import camera_pose  # noqa: E402

FOV = 0.6911112070083618
BBOX = (-2.0, -2.0, -2.0, 2.0, 2.0, 2.0)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


def alternate(cases, rounds, inner):
    """cases {name: fn}: one warm-up call each, then `rounds` rounds in which every case is timed once, in order."""
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in cases}
    for _ in range(rounds):
        for name, fn in cases.items():
            ms[name].append(timed(fn, inner))
    return {name: stats(v) for name, v in ms.items()}


def psnr_curve(script, extra, steps):
    """Run an example as a fresh process -> [(step, held-out PSNR dB, seconds of training so far)] from its table (ms per step times
    the steps of each row, summed: the evaluation between rows is not training time)."""
    cmd = [sys.executable, os.path.join(REPO, "examples", script), "--steps", str(steps)] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=300).stdout
    rows, seconds, last = [], 0.0, 0
    for m in re.finditer(r"^\s*(\d+)\s+\S+\s+([\d.]+) dB\s+([\d.]+)", out, re.M):
        step, db, ms = int(m.group(1)), float(m.group(2)), float(m.group(3))
        seconds += ms * 1e-3 * (step - last)
        last = step
        rows.append({"step": step, "psnr_dB": db, "train_seconds": seconds})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--example-steps", type=int, default=300)
    ap.add_argument("--example-views", type=int, default=64, help="training views of both examples (train_synthetic.py's default is 16)")
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hashfield_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_hashfield.py needs a GPU"
    assert args.rounds >= 5
    dev = "cuda"

    teacher = nerf.Network(); nerf.load_network(teacher, os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"))
    teacher = teacher.cuda().eval()
    t_ren = nerf.Renderer(teacher)
    rays_o, rays_d, colors = [], [], []
    with torch.no_grad():
        for v in range(64):
            o, d = nerf.generate_rays(camera_pose(360.0 * v / 64, elevation_deg=20.0 + 25.0 * (v % 3)), 200, 200, FOV, dev)
            rgb, _ = t_ren.render({"rays_o": o[None], "rays_d": d[None]})
            rays_o.append(o); rays_d.append(d); colors.append(rgb)
    O, D, C = torch.cat(rays_o), torch.cat(rays_d), torch.cat(colors)

    torch.manual_seed(0)
    field = nerf.HashField(BBOX).cuda()
    ren = nerf.HashRenderer(field)
    opt = FusedAdam(field.parameters(), lr=1e-2, eps=1e-15)
    gen = torch.Generator(device=dev).manual_seed(1)

    def batch():
        ids = torch.randint(0, O.shape[0], (4096,), device=dev, generator=gen)
        return O[ids].contiguous(), D[ids].contiguous(), C[ids].contiguous()
    for _ in range(args.train_steps):
        train_step(ren, opt, *batch())
    grid = field.occupancy_grid(N=args.grid, level=0.0, dilate=1)
    culled = nerf.HashRenderer(field)
    culled.occupancy, culled.stats = grid, []

    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "timer": "device events around whole render() / train_step() calls; rounds alternate the cases",
           "field": {"levels": 16, "log2_hashmap_size": 19, "width": 64, "samples_per_ray": 192, "trained_steps": args.train_steps,
                     "grid_points_per_axis": args.grid, "grid_occupied_fraction": grid.occupied_fraction("fine")}}

    # ---- an 800 x 800 frame
    o, d = nerf.generate_rays(camera_pose(40.0), 800, 800, FOV, dev)
    frame = {"rays_o": o[None], "rays_d": d[None]}
    mlp = {}
    for prec in ("f32", "f32x"):
        net = nerf.Network(); nerf.load_network(net, os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"))
        net = net.cuda().eval()
        net.precision = prec
        mlp[prec] = nerf.Renderer(net)

    def render(r):
        with torch.no_grad():
            return r.render(frame)
    rec["frame_800x800_ms"] = alternate({"hashfield": lambda: render(ren), "hashfield_grid": lambda: render(culled),
                                         "renderer_f32": lambda: render(mlp["f32"]), "renderer_f32x": lambda: render(mlp["f32x"])},
                                        args.rounds, 1)
    rec["field"]["frame_evaluated_fraction_with_grid"] = sum(m for m, _ in culled.stats) / max(1, sum(p for _, p in culled.stats))
    with torch.no_grad():
        a, b = ren.render(frame)[0], culled.render(frame)[0]
    rec["field"]["frame_max_abs_difference_with_grid"] = float((a - b).abs().max())
    print("frame", json.dumps(rec["frame_800x800_ms"]), flush=True)

    # ---- a 4096-ray training step
    fixed = batch()
    culled.stats = []
    steps = {"hashfield": lambda: train_step(ren, opt, *fixed), "hashfield_grid": lambda: train_step(culled, opt, *fixed)}
    for prec in ("f32", "f32x"):
        net = nerf.Network(); nerf.load_network(net, os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"))
        net = net.cuda().train()
        net.precision = prec
        r, o_mlp = nerf.Renderer(net), FusedAdam(net.parameters(), lr=5e-4)
        steps["renderer_" + prec] = (lambda r=r, o_mlp=o_mlp: train_step(r, o_mlp, *fixed))
    rec["train_step_4096_rays_ms"] = alternate(steps, args.rounds, 5)
    rec["field"]["step_evaluated_fraction_with_grid"] = sum(m for m, _ in culled.stats) / max(1, sum(p for _, p in culled.stats))
    print("step", json.dumps(rec["train_step_4096_rays_ms"]), flush=True)

    # ---- held-out PSNR against wall-clock seconds, each example a fresh process
    views = ["--views", str(args.example_views)]
    rec["psnr_over_time"] = {
        "what": "held-out PSNR of examples/train_hashfield.py and examples/train_synthetic.py (f32x) after the training seconds so far, "
                "both on the same number of teacher views",
        "views": args.example_views,
        "train_hashfield": psnr_curve("train_hashfield.py", views, args.example_steps),
        "train_hashfield_occupancy_64": psnr_curve("train_hashfield.py", views + ["--occupancy", "64"], args.example_steps),
        "train_synthetic_f32x": psnr_curve("train_synthetic.py", views + ["--precision", "f32x", "--out",
                                                                          tempfile.mkdtemp(prefix="nerf_train_")], args.example_steps)}
    print("psnr", json.dumps(rec["psnr_over_time"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
