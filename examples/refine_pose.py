#!/usr/bin/env python3
"""Recover a perturbed camera pose by gradient descent through the renderer (iNeRF-style pose estimation).

A frozen network (tests/golden/trained_ckpt.pth) renders a target view.  The camera is then moved by a few degrees and a few
centimetres, and a 6-DoF correction (axis-angle + translation, one torch leaf) is optimised with Adam through
Renderer.render: the rays are built from the corrected pose in torch, so rays_o / rays_d require grad and the HIP backward
returns d loss / d rays (no parameter gradient is computed: the network is frozen).

    python examples/refine_pose.py --steps 300 --rays 2048 --precision f32x

Prints the pose error every few steps and the median ms per step (forward + backward + Adam).  Needs an MI355X and the built
library (python -c "import __graft_entry__ as g; g.build()")."""
import argparse
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "examples"))
import nerf_replication_amd as nerf  # noqa: E402
from render_frame import camera_pose  # noqa: E402

FOV = 0.6911112070083618


def skew(w):
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def so3_exp(w):
    """Rodrigues' formula; its series form near w = 0 (where the correction starts) keeps the gradient finite."""
    th2 = (w * w).sum()
    K = skew(w)
    eye = torch.eye(3, dtype=w.dtype, device=w.device)
    if float(th2.detach()) < 1e-12:
        return eye + K + 0.5 * K @ K
    th = th2.sqrt()
    return eye + (torch.sin(th) / th) * K + ((1 - torch.cos(th)) / th2) * K @ K


def rotation_error_deg(Ra, Rb):
    c = ((Ra.T @ Rb).trace() - 1.0) / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, float(c)))))


def camera_dirs(H, W, pixel_ids, device):
    """Unnormalised pinhole directions in the camera frame (the formula of nerf_generate_rays / blender.py:102-127)."""
    f = W / (2.0 * math.tan(FOV / 2.0))
    u, v = (pixel_ids % W).double(), (pixel_ids // W).double()
    return torch.stack([(u - W / 2.0) / f, -(v - H / 2.0) / f, -torch.ones_like(u)], -1).float().to(device)


def rays_from_pose(R, t, dirs):
    d = dirs @ R.T
    d = d / d.norm(dim=-1, keepdim=True)
    return t.expand_as(d), d


def refine(ckpt=os.path.join(REPO, "tests", "golden", "trained_ckpt.pth"), precision="f32", steps=300, n_rays=2048, res=200,
           angle=40.0, elevation=45.0, rot_deg=3.0, trans=0.05, lr=3e-3, seed=0, log_every=0, object_only=True):
    """-> dict(rot_err_deg, trans_err: per step, index 0 = the perturbed start; ms_per_step: median after 5 warm-up steps)."""
    dev = "cuda"
    net = nerf.Network()
    nerf.load_network(net, ckpt)
    net = net.cuda().eval().requires_grad_(False)
    net.precision = precision
    ren = nerf.Renderer(net)
    c2w = camera_pose(angle, elevation_deg=elevation)
    R_true, t_true = c2w[:3, :3].to(dev), c2w[:3, 3].to(dev)

    # target: the frozen network's own view; rays on the object (not the white background) carry the pose signal
    gen = torch.Generator().manual_seed(seed)
    ids_all = torch.arange(res * res)
    with torch.no_grad():
        o, d = rays_from_pose(R_true, t_true, camera_dirs(res, res, ids_all, dev))
        full, _ = ren.render({"rays_o": o[None], "rays_d": d[None]})
    on_obj = ids_all[(full.min(1).values < 0.95).cpu()]
    pool = on_obj if object_only and on_obj.numel() >= n_rays else ids_all
    ids = pool[torch.randperm(pool.numel(), generator=gen)[:n_rays]]
    dirs = camera_dirs(res, res, ids, dev)
    target = full[ids.to(dev)]

    # perturbation: rot_deg about a random axis, `trans` (scene units) in a random direction
    ax = torch.randn(3, generator=gen); ax = ax / ax.norm()
    dt = torch.randn(3, generator=gen); dt = dt / dt.norm()
    R0 = so3_exp((math.radians(rot_deg) * ax).to(dev)) @ R_true
    t0 = t_true + trans * dt.to(dev)

    xi = torch.zeros(6, device=dev, requires_grad=True)        # (axis-angle, translation) correction of the perturbed pose
    opt = torch.optim.Adam([xi], lr=lr)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.1 ** (1.0 / max(1, steps)))
    rot_err, trans_err, times = [], [], []

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
        record()
        if log_every and (step + 1) % log_every == 0:
            print("{:5d}  loss {:.3e}  rotation error {:6.3f} deg  translation error {:7.4f}".format(
                step + 1, loss.item(), rot_err[-1], trans_err[-1]))
    warm = sorted(times[min(5, len(times) - 1):])
    return dict(rot_err_deg=rot_err, trans_err=trans_err, ms_per_step=warm[len(warm) // 2], n_rays=int(ids.numel()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=os.path.join(REPO, "tests", "golden", "trained_ckpt.pth"))
    ap.add_argument("--precision", default="f32", choices=["f32", "f32x"])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--rot-deg", type=float, default=3.0)
    ap.add_argument("--trans", type=float, default=0.05)
    args = ap.parse_args()
    r = refine(args.ckpt, args.precision, args.steps, args.rays, rot_deg=args.rot_deg, trans=args.trans, log_every=25)
    print("start: rotation error {:.3f} deg, translation error {:.4f}".format(r["rot_err_deg"][0], r["trans_err"][0]))
    print("end:   rotation error {:.3f} deg, translation error {:.4f}".format(r["rot_err_deg"][-1], r["trans_err"][-1]))
    print("{} rays, {}: {:.2f} ms/step (median; render + backward + Adam)".format(r["n_rays"], args.precision, r["ms_per_step"]))


if __name__ == "__main__":
    main()
