#!/usr/bin/env python3
"""Times the deformation field of a dynamic scene in one process on one GPU:

  * nerf_deform_forward and nerf_deform_backward alone at 2^20 rows (T = 32, R = 256, no canonical ray, every clamp open or shut as
    random tables leave it), nerf_deform_pack and nerf_deform_unpack_grad, against the eager-torch restatement of the reference's
    compute_delta (nine grid_sample planes, stacks and products over [3, 64, M] temporaries; tests/test_gpu_deform.py's
    eager_delta) -- forward under no_grad, and forward + backward of sum(x_warped * g);
  * an 800 x 800 frame and a 4096-ray training step (train_step with FusedAdam) of a dynamic HashField against the same field's
    static twin (the same hash encoder and heads without the warp), alternately.

Device events around whole calls, a warm-up of every case, then alternating rounds; median with min-max (tools/time_hashfield.py's
helpers).  Writes profiles/deform_timing.json.  No speed is asserted.  Needs an MI355X and the built library.

    python tools/time_deform.py [--rounds 7] [--rows 1048576] [--frames 32] [--reso 256]
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
from time_hashfield import BBOX, FOV, alternate  # noqa: E402
from test_gpu_deform import eager_delta  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reso", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deform_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_deform.py needs a GPU"
    assert args.rounds >= 5
    dev, call = "cuda", nerf._lib.call
    M, T, Rr, S = args.rows, args.frames, args.reso, 128
    n = M // S
    torch.manual_seed(0)
    dn = nerf.DNeRFNGP(T, reso=Rr, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                       desired_resolution=2048).cuda()                              # HashField's default encoder under the warp
    feat = [f.detach() for f in dn.feat]
    packed = dn.packed()
    x = torch.rand(M, 3, device=dev)
    time = 0.5 + torch.rand(n, device=dev) * (T - 1.5)                               # no canonical ray
    t_rows = time.repeat_interleave(S)
    g = torch.randn(M, 3, device=dev)
    out, g_packed = torch.empty(M, 3, device=dev), torch.zeros_like(packed)
    grads = [torch.empty_like(f) for f in feat]
    leaves = [f.clone().requires_grad_() for f in feat]

    def eager_forward(tables):
        return torch.clamp(x + eager_delta(tables, x, t_rows, T), 0.0, 1.0)

    def eager_step():
        for f in leaves:
            f.grad = None
        (eager_forward(leaves) * g).sum().backward()

    def no_grad_eager():
        with torch.no_grad():
            eager_forward(feat)

    def hip_step():
        g_packed.zero_()
        call("nerf_deform_forward", x, time, None, M, n, S, packed, 64, T, Rr, out, None)
        call("nerf_deform_backward", x, time, None, M, n, S, packed, 64, T, Rr, g, None, g_packed)
        call("nerf_deform_unpack_grad", g_packed, 64, T, Rr, grads)
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "rows": M, "frames": T, "reso": Rr,
           "timer": "device events around whole calls; rounds alternate the cases"}
    rec["kernels_ms"] = alternate({
        "hip_forward": lambda: call("nerf_deform_forward", x, time, None, M, n, S, packed, 64, T, Rr, out, None),
        "hip_backward": lambda: call("nerf_deform_backward", x, time, None, M, n, S, packed, 64, T, Rr, g, None, g_packed),
        "hip_pack": lambda: call("nerf_deform_pack", feat, 64, T, Rr, packed),
        "hip_unpack_grad": lambda: call("nerf_deform_unpack_grad", g_packed, 64, T, Rr, grads),
        "hip_forward_backward": hip_step,
        "eager_forward": no_grad_eager,
        "eager_forward_backward": eager_step}, args.rounds, 3)
    k = rec["kernels_ms"]
    tap_bytes = M * 36 * 256
    rec["derived"] = {
        "tap_bytes_per_call": tap_bytes,
        "forward_gathered_TB_per_s": tap_bytes / (k["hip_forward"]["median"] * 1e-3) / 1e12,
        "backward_atomic_added_TB_per_s_upper": tap_bytes / (k["hip_backward"]["median"] * 1e-3) / 1e12,
        "what": "36 rows of 256 B per sample; the backward's figure counts every tap as added (an upper figure: coordinates whose "
                "clamp is shut add nothing) and its time holds the 36 gathers of the recomputed forward as well",
        "forward_speedup_over_eager": k["eager_forward"]["median"] / k["hip_forward"]["median"],
        "forward_backward_speedup_over_eager": k["eager_forward_backward"]["median"] / k["hip_forward_backward"]["median"]}
    print("kernels", json.dumps({a: b["median"] for a, b in k.items()}), json.dumps(rec["derived"]), flush=True)
    del leaves

    # a dynamic field and its static twin: the same hash encoder (shared) and the same heads
    dyn = nerf.HashField(BBOX, encoder=dn).cuda()
    twin = nerf.HashField(BBOX, encoder=dn.encoder).cuda()
    twin.sigma_net.load_state_dict(dyn.sigma_net.state_dict())
    twin.color_net.load_state_dict(dyn.color_net.state_dict())
    rens = {"dynamic": nerf.HashRenderer(dyn), "static_twin": nerf.HashRenderer(twin)}
    opts = {name: FusedAdam(r.field.parameters(), lr=1e-3, eps=1e-15) for name, r in rens.items()}
    o, d = nerf.generate_rays(camera_pose(40.0), 800, 800, FOV, dev)
    frame = {"rays_o": o[None], "rays_d": d[None], "time": torch.full((1,), 0.5 * (T - 1), device=dev)}

    def render(r):
        with torch.no_grad():
            return r.render(frame)
    rec["frame_800x800_ms"] = alternate({name: (lambda r=r: render(r)) for name, r in rens.items()}, args.rounds, 1)
    print("frame", json.dumps({a: b["median"] for a, b in rec["frame_800x800_ms"].items()}), flush=True)
    ids = torch.randint(0, o.shape[0], (4096,), device=dev)
    so, sd = o[ids].contiguous(), d[ids].contiguous()
    colors = torch.rand(4096, 3, device=dev)
    step_time = 0.5 + torch.rand(4096, device=dev) * (T - 1.5)
    rec["train_step_4096_rays_ms"] = alternate({
        "dynamic": lambda: train_step(rens["dynamic"], opts["dynamic"], so, sd, colors, time=step_time),
        "static_twin": lambda: train_step(rens["static_twin"], opts["static_twin"], so, sd, colors)}, args.rounds, 5)
    print("step", json.dumps({a: b["median"] for a, b in rec["train_step_4096_rays_ms"].items()}), flush=True)
    rec["field"] = {"levels": 16, "log2_hashmap_size": 19, "width": 64, "samples_per_ray": 192, "trained_steps": 0,
                    "frame_time": 0.5 * (T - 1), "step_times": "uniform in [0.5, T - 1]"}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
