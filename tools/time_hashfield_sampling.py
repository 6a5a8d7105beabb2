#!/usr/bin/env python3
"""Times the hash field's sampling choices (HashRenderer.N_samples / N_importance / perturb) against each other
in one process on one GPU: for every configuration (default 192 uniform, 64 + 64, 32 + 64, 64 + 128) an 800 x 800 frame and a 4096-ray
training step (train_step with FusedAdam, perturb on), run alternately, and the sampler's own share of a chunk:
nerf_field_sample_importance alone on the weights of a 16384-ray chunk of the frame and of the 4096 rays of the step.  Device events
around whole calls, a warm-up of every case, then alternating rounds; median with min-max: the method of tools/time_hashfield.py, whose
helpers this tool uses.  The field is first trained for --train-steps steps on 64 + 64 with perturb, so that the weights have a surface to
find.  Then examples/train_hashfield.py runs as fresh processes, every configuration with and without --perturb, and the held-out PSNR
after the same number of steps is recorded.  Merges its record into profiles/hashfield_sampling.json under "timing" (the parity figures
and the training bound of the tests live in the same file).  Needs an MI355X and the built library.

    python tools/time_hashfield_sampling.py [--rounds 7] [--train-steps 300] [--example-steps 300] [--configs 192+0,64+64,32+64,64+128]

No speed is asserted.  A coarse pass costs Sc density evaluations on top of the Sc + Sf full ones, so a configuration can lose against
the uniform table; whatever comes out is recorded.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "examples"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)
import nerf_replication_amd as nerf  # noqa: E402
from nerf_replication_amd.training import FusedAdam, train_step  # noqa: E402
from render_frame import camera_pose  # noqa: E402
from time_hashfield import BBOX, FOV, alternate, psnr_curve, stats, timed  # noqa: E402
import hashfield_sampling_reference as SR  # noqa: E402


def renderer(field, Sc, Sf, perturb):
    ren = nerf.HashRenderer(field)
    ren.N_samples, ren.N_importance, ren.perturb = Sc, Sf, perturb
    return ren


def sampler_alone(ren, batch, rounds):
    """ms of nerf_field_sample_importance alone on the first chunk of `batch`, from the (t_coarse, weights, t_merged) `samples` hands
    out -> stats, or None without resampling."""
    if ren.N_importance == 0:
        return None
    ren.samples = []
    with torch.no_grad():
        ren.render(batch)
    t_c, w, t_m = ren.samples[0]
    ren.samples = None
    n, Sc, Sf = w.shape[0], ren.N_samples, ren.N_importance
    u = torch.rand(n, Sf, device=w.device) if ren.perturb else torch.linspace(0.0, 1.0, Sf).to(w.device)
    out = torch.empty_like(t_m)

    def run():
        nerf._lib.call("nerf_field_sample_importance", w, t_c, 0 if t_c.dim() == 1 else Sc, u, 0 if u.dim() == 1 else Sf, n, Sc, Sf,
                       out, None)
    run()
    torch.cuda.synchronize()
    return dict(stats([timed(run, 20) for _ in range(rounds)]), rays=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--example-steps", type=int, default=300)
    ap.add_argument("--example-views", type=int, default=64)
    ap.add_argument("--configs", default="192+0,64+64,32+64,64+128")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_hashfield_sampling.py needs a GPU"
    assert args.rounds >= 5
    configs = [tuple(int(v) for v in c.split("+")) for c in args.configs.split(",")]
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
    opt = FusedAdam(field.parameters(), lr=1e-2, eps=1e-15)
    gen = torch.Generator(device=dev).manual_seed(1)

    def batch():
        ids = torch.randint(0, O.shape[0], (4096,), device=dev, generator=gen)
        return O[ids].contiguous(), D[ids].contiguous(), C[ids].contiguous()
    warm = renderer(field, 64, 64, True)
    for _ in range(args.train_steps):
        train_step(warm, opt, *batch())

    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "timer": "device events around whole render() / train_step() calls; rounds alternate the configurations",
           "field": {"levels": 16, "log2_hashmap_size": 19, "width": 64, "trained_steps": args.train_steps, "trained_on": "64+64 perturb"},
           "configurations": ["%d+%d" % c for c in configs]}

    o, d = nerf.generate_rays(camera_pose(40.0), 800, 800, FOV, dev)
    frame = {"rays_o": o[None], "rays_d": d[None]}
    eval_rens = {"%d+%d" % c: renderer(field, c[0], c[1], False) for c in configs}
    train_rens = {"%d+%d" % c: renderer(field, c[0], c[1], True) for c in configs}

    def render(r):
        with torch.no_grad():
            return r.render(frame)
    rec["frame_800x800_ms"] = alternate({k: (lambda r=r: render(r)) for k, r in eval_rens.items()}, args.rounds, 1)
    print("frame", json.dumps(rec["frame_800x800_ms"]), flush=True)
    fixed = batch()
    rec["train_step_4096_rays_ms"] = alternate({k: (lambda r=r: train_step(r, opt, *fixed)) for k, r in train_rens.items()},
                                               args.rounds, 5)
    print("step", json.dumps(rec["train_step_4096_rays_ms"]), flush=True)
    step_batch = {"rays_o": fixed[0][None], "rays_d": fixed[1][None]}
    rec["sampler_alone_ms"] = {
        "what": "nerf_field_sample_importance alone: on the first 16384-ray chunk of the frame (shared u) and on the 4096 rays of the "
                "step (random u per ray)",
        "frame_chunk": {k: sampler_alone(r, frame, args.rounds) for k, r in eval_rens.items()},
        "train_step": {k: sampler_alone(r, step_batch, args.rounds) for k, r in train_rens.items()}}
    print("sampler", json.dumps(rec["sampler_alone_ms"]), flush=True)

    views = ["--views", str(args.example_views)]
    rec["held_out_psnr"] = {"what": "examples/train_hashfield.py as fresh processes, %d steps on %d teacher views of 200 x 200; the last "
                                    "row of each table" % (args.example_steps, args.example_views)}
    for Sc, Sf in configs:
        for perturb in (False, True):
            extra = views + ["--n-samples", str(Sc), "--importance", str(Sf)] + (["--perturb"] if perturb else [])
            rows = psnr_curve("train_hashfield.py", extra, args.example_steps)
            rec["held_out_psnr"]["%d+%d%s" % (Sc, Sf, " perturb" if perturb else "")] = rows[-1] if rows else None
            print("psnr", Sc, Sf, perturb, json.dumps(rows[-1] if rows else None), flush=True)
    SR.record("timing", rec)
    print("wrote", SR.SAMPLING_JSON)


if __name__ == "__main__":
    main()
