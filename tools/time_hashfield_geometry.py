#!/usr/bin/env python3
"""Times the hash field's geometry outputs and ray gradients against its plain render, in one process on
one GPU, with the method of tools/time_hashfield.py (device events around whole calls, a warm-up of every case, alternating rounds,
every sample kept, median with min-max):

    an 800 x 800 frame at 192 samples per ray     HashRenderer.render against HashRenderer.render_geometry, without and with a 128^3
                                                  occupancy grid of the field itself
    a 4096-ray step (render, MSE, backward)       ray_gradients off (parameter gradients) against on (rays that require grad:
                                                  parameter and ray gradients of one call), and train_step with FusedAdam

The field is first trained for --train-steps steps against the teacher, as tools/time_hashfield.py does.  --baseline-module PATH
takes a copy of an earlier nerf_replication_amd/hashfield.py (the parent commit's): it is loaded next to the package's own and its
render / train_step are timed IN THE SAME ROUNDS on a field that holds the very same parameter tensors, so that "the plain path did
not move" is a comparison inside one session (the record says whether the new medians lie inside the baseline's min-max).  No bound
is asserted.
Writes profiles/hashfield_geometry_timing.json.  Needs an MI355X and the built library.

    python tools/time_hashfield_geometry.py [--rounds 7] [--train-steps 300] [--baseline-module old_hashfield.py] [--out ...]
"""
import argparse
import importlib.util
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "examples"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import nerf_replication_amd as nerf  # noqa: E402
from nerf_replication_amd.training import FusedAdam, train_step  # noqa: E402
from render_frame import camera_pose  # noqa: E402
from time_hashfield import BBOX, FOV, alternate  # noqa: E402


def load_baseline(path):
    spec = importlib.util.spec_from_file_location("nerf_replication_amd.hashfield_baseline", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def share_state(dst, src):
    """Make dst's parameters and buffers the very tensors of src: both fields then read the same memory, and a difference between
    their timings is a difference of the code that runs, not of where an allocation landed."""
    for store in ("_parameters", "_buffers"):
        names = src.named_parameters() if store == "_parameters" else src.named_buffers()
        for name, t in names:
            *path, leaf = name.split(".")
            mod = dst
            for part in path:
                mod = getattr(mod, part)
            getattr(mod, store)[leaf] = t


def inside(new, old):
    return old["min"] <= new["median"] <= old["max"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--baseline-module", default=None, metavar="PATH", help="a copy of an earlier nerf_replication_amd/hashfield.py")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hashfield_geometry_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_hashfield_geometry.py needs a GPU"
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
    culled.occupancy = grid

    base = base_ren = base_culled = base_opt = None
    if args.baseline_module:
        base = load_baseline(args.baseline_module)
        base_field = base.HashField(BBOX)
        share_state(base_field, field)
        base_ren, base_culled = base.HashRenderer(base_field), base.HashRenderer(base_field)
        base_culled.occupancy = grid
        base_opt = opt                                  # the same parameters: the same optimizer state

    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "timer": "device events around whole calls; rounds alternate the cases",
           "baseline_module": bool(base),
           "field": {"levels": 16, "log2_hashmap_size": 19, "width": 64, "samples_per_ray": 192, "trained_steps": args.train_steps,
                     "grid_points_per_axis": args.grid, "grid_occupied_fraction": grid.occupied_fraction("fine"),
                     "geometry_chunk_rays": ren.geometry_chunk_rays}}

    # ---- an 800 x 800 frame
    o, d = nerf.generate_rays(camera_pose(40.0), 800, 800, FOV, dev)
    frame = {"rays_o": o[None], "rays_d": d[None]}

    def render(r):
        with torch.no_grad():
            return r.render(frame)
    cases = {"render": lambda: render(ren), "render_grid": lambda: render(culled),
             "render_geometry": lambda: ren.render_geometry(frame), "render_geometry_grid": lambda: culled.render_geometry(frame)}
    if base:
        cases.update({"baseline_render": lambda: render(base_ren), "baseline_render_grid": lambda: render(base_culled)})
    rec["frame_800x800_ms"] = alternate(cases, args.rounds, 1)
    print("frame", json.dumps({k: v["median"] for k, v in rec["frame_800x800_ms"].items()}), flush=True)

    # ---- a 4096-ray step
    fixed = batch()
    on = nerf.HashRenderer(field)
    on.ray_gradients = True

    def step(r, rays_need_grad):
        o4, d4 = fixed[0][None], fixed[1][None]
        if rays_need_grad:
            o4, d4 = o4.clone().requires_grad_(True), d4.clone().requires_grad_(True)
        for p in r.field.parameters():
            p.grad = None
        rgb, _ = r.render({"rays_o": o4, "rays_d": d4})
        torch.nn.functional.mse_loss(rgb, fixed[2]).backward()
    steps = {"backward_ray_gradients_off": lambda: step(ren, False), "backward_ray_gradients_on": lambda: step(on, True),
             "train_step": lambda: train_step(ren, opt, *fixed)}
    if base:
        steps.update({"baseline_backward": lambda: step(base_ren, False), "baseline_train_step": lambda: train_step(base_ren, base_opt, *fixed)})
    rec["step_4096_rays_ms"] = alternate(steps, args.rounds, 5)
    print("step", json.dumps({k: v["median"] for k, v in rec["step_4096_rays_ms"].items()}), flush=True)

    if base:
        f, s = rec["frame_800x800_ms"], rec["step_4096_rays_ms"]
        rec["plain_path_inside_baseline_min_max"] = {
            "render": inside(f["render"], f["baseline_render"]), "render_grid": inside(f["render_grid"], f["baseline_render_grid"]),
            "backward": inside(s["backward_ray_gradients_off"], s["baseline_backward"]),
            "train_step": inside(s["train_step"], s["baseline_train_step"])}
        print("plain path inside the baseline's min-max:", json.dumps(rec["plain_path_inside_baseline_min_max"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
