#!/usr/bin/env python3
"""Recover a perturbed camera pose by gradient descent through HashRenderer.render: examples/refine_pose.py on a hash-grid radiance
field.

A frozen HashField (the state dict examples/train_hashfield.py --out writes) renders a target view.  The camera is then moved by a few
degrees and a few centimetres, and a 6-DoF correction (axis-angle + translation, one torch leaf) is optimised with Adam through
HashRenderer.render with ray_gradients = True: the rays are built from the corrected pose in torch, so rays_o / rays_d require grad
and the HIP backward returns d loss / d rays (no parameter gradient is computed: the field is frozen).

    python examples/train_hashfield.py --steps 600 --out field.pth
    python examples/refine_hashfield_pose.py --field field.pth --steps 300 --rays 2048

--levels / --log2-hashmap-size must be those the field was trained with (the state dict holds the tables, not the encoder's
arguments; the box travels in it).  Prints the pose error every few steps and the median ms per step (forward + backward + Adam)."""
import argparse
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "examples"))
import nerf_replication_amd as nerf  # noqa: E402
from refine_pose import camera_dirs, rays_from_pose, rotation_error_deg, so3_exp  # noqa: E402
from render_frame import camera_pose  # noqa: E402


def load_field(path, levels=16, log2_hashmap_size=19):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    encoder = nerf.HashEncoder(input_dim=3, num_levels=levels, level_dim=2, base_resolution=16, log2_hashmap_size=log2_hashmap_size,
                               desired_resolution=2048)
    field = nerf.HashField(sd["wbounds"].tolist(), encoder=encoder)
    field.load_state_dict(sd, strict=True)
    return field


def refine(field, steps=300, n_rays=2048, res=200, samples=192, angle=40.0, elevation=45.0, rot_deg=3.0, trans=0.05, lr=3e-3, seed=0,
           log_every=0, object_only=True):
    """-> dict(loss, rot_err_deg, trans_err: per step, the errors with index 0 = the perturbed start; ms_per_step: median after 5
    warm-up steps)."""
    dev = "cuda"
    field = field.cuda().eval().requires_grad_(False)
    ren = nerf.HashRenderer(field)
    ren.N_samples, ren.ray_gradients = samples, True
    c2w = camera_pose(angle, elevation_deg=elevation)
    R_true, t_true = c2w[:3, :3].to(dev), c2w[:3, 3].to(dev)

    # target: the frozen field's own view; rays on the object (not the white background) carry the pose signal
    gen = torch.Generator().manual_seed(seed)
    ids_all = torch.arange(res * res)
    with torch.no_grad():
        o, d = rays_from_pose(R_true, t_true, camera_dirs(res, res, ids_all, dev))
        full, _ = ren.render({"rays_o": o[None].contiguous(), "rays_d": d[None]})
    on_obj = ids_all[(full.min(1).values < 0.95).cpu()]
    pool = on_obj if object_only and on_obj.numel() >= n_rays else ids_all
    ids = pool[torch.randperm(pool.numel(), generator=gen)[:n_rays]]
    dirs = camera_dirs(res, res, ids, dev)
    target = full[ids.to(dev)]

    ax = torch.randn(3, generator=gen); ax = ax / ax.norm()
    dt = torch.randn(3, generator=gen); dt = dt / dt.norm()
    R0 = so3_exp((math.radians(rot_deg) * ax).to(dev)) @ R_true
    t0 = t_true + trans * dt.to(dev)

    xi = torch.zeros(6, device=dev, requires_grad=True)        # (axis-angle, translation) correction of the perturbed pose
    opt = torch.optim.Adam([xi], lr=lr)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.1 ** (1.0 / max(1, steps)))
    losses, rot_err, trans_err, times = [], [], [], []

    def record():
        with torch.no_grad():
            R, t = so3_exp(xi[:3]) @ R0, t0 + xi[3:]
            rot_err.append(rotation_error_deg(R, R_true))
            trans_err.append(float((t - t_true).norm()))

    record()
    for step in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        R, t = so3_exp(xi[:3]) @ R0, t0 + xi[3:]
        o, d = rays_from_pose(R, t, dirs)
        rgb, _ = ren.render({"rays_o": o[None], "rays_d": d[None]})
        loss = torch.nn.functional.mse_loss(rgb, target)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        sched.step()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
        losses.append(float(loss.detach()))
        record()
        if log_every and (step + 1) % log_every == 0:
            print("{:5d}  loss {:.3e}  rotation error {:6.3f} deg  translation error {:7.4f}".format(
                step + 1, losses[-1], rot_err[-1], trans_err[-1]))
    warm = sorted(times[min(5, len(times) - 1):])
    return dict(loss=losses, rot_err_deg=rot_err, trans_err=trans_err, ms_per_step=warm[len(warm) // 2], n_rays=int(ids.numel()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", required=True, help="a state dict written by examples/train_hashfield.py --out")
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--log2-hashmap-size", type=int, default=19)
    ap.add_argument("--samples", type=int, default=192, help="depths per ray (HashRenderer.N_samples, 1..192)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--rot-deg", type=float, default=3.0)
    ap.add_argument("--trans", type=float, default=0.05)
    args = ap.parse_args()
    field = load_field(args.field, args.levels, args.log2_hashmap_size)
    r = refine(field, args.steps, args.rays, samples=args.samples, rot_deg=args.rot_deg, trans=args.trans, log_every=25)
    print("start: rotation error {:.3f} deg, translation error {:.4f}".format(r["rot_err_deg"][0], r["trans_err"][0]))
    print("end:   rotation error {:.3f} deg, translation error {:.4f}".format(r["rot_err_deg"][-1], r["trans_err"][-1]))
    print("loss {:.3e} -> {:.3e}".format(r["loss"][0], r["loss"][-1]))
    print("{} rays: {:.2f} ms/step (median; render + backward + Adam)".format(r["n_rays"], r["ms_per_step"]))
    if not r["loss"][-1] < r["loss"][0]:
        sys.exit("the loss did not fall below its start value")


if __name__ == "__main__":
    main()
