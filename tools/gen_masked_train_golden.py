"""Generate tests/golden/masked_train.npz by running the REAL reference on CPU under autograd in the two modes that
tools/gen_stochastic_golden.py and oracle/gen_golden.py do not cover: fast_sampling (the ESS / ERT masked fine pass) and
N_importance = 0 (coarse only).  Deterministic sampling (task "test").  Like its siblings it needs the reference checkout,
runs in the build container only and copies no reference source (import recipe, npz writer: oracle/gen_golden.py).

    python tools/gen_masked_train_golden.py        # rewrites the file below, bit-identically

Cases, 96 pinhole rays each (pose 40 deg), target = the sharp family's plain render of the same rays:
  trained_t002   trained_ckpt.pth, weights_threshold 0.02   (a useful mask)
  sharp_t025     sharp family, 0.25 (the reference default)
  trained_t025   trained_ckpt.pth, 0.25: no fine sample is valid, the fine network sees the 64 coarse depths of every ray
  coarse_only    trained_ckpt.pth, ren.N_importance = 0 on the reference instance
Per case: rays, pixel ids, target, coarse sigma (pre-ReLU), valid_fine [n,128] (sampler order) and valid_sorted [n,192]
(masked cases), t_sorted, rgb, depth, loss and the gradients of every parameter that has one (weight matrices as a flat
stride-53 subsample: 53 is coprime to every row length 63, 128, 256, 283, 319; the file stays under 1 MiB).

The mask is a set of threshold comparisons on the coarse weights, so a last-bit difference in the coarse sigma can flip a bit
of it -- the reference's own discontinuity.  A test of another implementation must not hide a defect behind that, so only
rays whose reference mask does not change under STABILITY_DRAWS seeded uniform perturbations of the coarse sigma (pre-ReLU)
of amplitude AMPLITUDE_REL x (max - min of the candidates' coarse sigma) are kept; candidates are drawn in a seeded order
until 96 remain.  AMPLITUDE_REL is ten times the worst coarse-sigma deviation (relative to the range) recorded for the HIP
path in profiles/parity_r03.json (2.3e-6, f32 and f32x).  The tests then ask for exact mask equality on every fixture ray.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import gen_golden as gg  # noqa: E402  (import_reference, npz, OUT)
import nerf_oracle as orc  # noqa: E402

N_RAYS = 96
POOL = 192                  # candidates examined at a time
AMPLITUDE_REL = 2.3e-5
STABILITY_DRAWS = 8
SEED = 11
GRAD_STRIDE = 53
POSE_DEG = 40.0


def _subsample(t):
    f = t.detach().reshape(-1)
    return f.clone() if f.numel() <= 4096 else f[::GRAD_STRIDE].clone()


def _net(Network, sd, train):
    net = Network()
    net.load_state_dict({k: sd[k].clone() for k in orc.state_dict_keys()}, strict=True)
    net.train() if train else net.eval()
    return net


def _quiet(fn, *args, **kwargs):
    """The reference prints its filter statistics on every masked call."""
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def _coarse_sigma(net, ren, o, d):
    t_c, pts_c = ren.stratified_sample_points_from_rays(o, d, N_samples=64, perturb=False)
    vd = d / torch.norm(d, dim=-1, keepdim=True)
    return t_c, net.forward(pts_c, vd, None, model="")[..., 3]


def _mask(ren, sigma_raw, o, d, t_c, thr):
    _, t_f, vm = _quiet(ren.fine_sample_points, torch.relu(sigma_raw), o, d, t_c, 128, 64, thr)
    return t_f, vm


def stable_rays(net, ren, thr, case_seed):
    """Pixel ids of the first N_RAYS candidates (seeded order) whose mask survives the perturbations, and the amplitude."""
    order = torch.from_numpy(np.random.default_rng(case_seed).permutation(800 * 800))
    c2w = orc.camera_pose(POSE_DEG)
    gen = torch.Generator().manual_seed(case_seed)
    kept, amplitude, seen = [], None, 0
    with torch.no_grad():
        while len(kept) < N_RAYS:
            ids = order[seen:seen + POOL]
            seen += POOL
            o, d = orc.pinhole_rays(800, 800, c2w, pixel_ids=ids)
            t_c, sig = _coarse_sigma(net, ren, o, d)
            if amplitude is None:       # fixed by the first pool, so that later pools cannot change earlier decisions
                amplitude = AMPLITUDE_REL * (sig.max() - sig.min()).item()
            _, vm0 = _mask(ren, sig, o, d, t_c, thr)
            ok = torch.ones(ids.shape[0], dtype=torch.bool)
            for _ in range(STABILITY_DRAWS):
                noise = (torch.rand(sig.shape, generator=gen) * 2 - 1) * amplitude
                _, vm = _mask(ren, sig + noise, o, d, t_c, thr)
                ok &= (vm == vm0).all(dim=1)
            print(f"    pool of {ids.shape[0]}: {int((~ok).sum())} rays with an unstable mask")
            kept.extend(ids[ok].tolist())
    return torch.tensor(kept[:N_RAYS], dtype=torch.int64), amplitude


def case(Network, Renderer, tag, sd, teacher_ren, thr, case_seed, coarse_only=False):
    net = _net(Network, sd, train=True)
    ren = Renderer(net)
    ren.device = torch.device("cpu")
    assert ren.perturb is False and ren.task != "train"
    rec = {}
    if coarse_only:
        ren.N_importance = 0
        ids = torch.from_numpy(np.random.default_rng(case_seed).choice(800 * 800, N_RAYS, replace=False))
    else:
        ren.fast_sampling, ren.weights_threshold = True, thr
        ids, amplitude = stable_rays(net, ren, thr, case_seed)
        rec.update(amplitude=amplitude, weights_threshold=thr)
    o, d = orc.pinhole_rays(800, 800, orc.camera_pose(POSE_DEG), pixel_ids=ids)
    with torch.no_grad():
        target, _ = teacher_ren.render({"rays_o": o[None], "rays_d": d[None]})
        t_c, sig = _coarse_sigma(net, ren, o, d)
    rgb, dep = _quiet(ren.render, {"rays_o": o[None], "rays_d": d[None]})
    loss = torch.nn.MSELoss()(rgb, target)
    net.zero_grad()
    loss.backward()
    rec.update(rays_o=o, rays_d=d, pixel_ids=ids, target=target, sigma_coarse_raw=sig, rgb=rgb.detach(), depth=dep.detach(),
               loss=loss.detach())
    if coarse_only:
        rec["t_sorted"] = t_c
    else:
        with torch.no_grad():
            t_f, vm = _mask(ren, sig, o, d, t_c, thr)
            t_sorted, idx = torch.sort(torch.cat([t_c, t_f], 1), dim=-1)
            valid = torch.gather(torch.cat([torch.ones(N_RAYS, 64, dtype=torch.bool), vm], 1), 1, idx)
        rec.update(valid_fine=vm.to(torch.uint8), valid_sorted=valid.to(torch.uint8), t_sorted=t_sorted)
        print(f"  [{tag}] fine samples valid: {vm.float().mean().item():.4f}")
    n_grad = 0
    for k, p in net.named_parameters():
        if p.grad is not None:
            rec["grad/" + k] = _subsample(p.grad)
            n_grad += 1
    assert n_grad == (24 if coarse_only else 48), n_grad
    print(f"  [{tag}] loss {loss.item():.8f}, {n_grad} gradients")
    return {f"{tag}/{k}": v for k, v in rec.items()}


def main():
    torch.set_num_threads(8)
    Network, Renderer = gg.import_reference()
    base = torch.load(os.path.join(gg.OUT, "synthetic_ckpt.pth"), weights_only=True)["net"]
    base = {k: base[k] for k in orc.state_dict_keys()}
    trained = torch.load(os.path.join(gg.OUT, "trained_ckpt.pth"), weights_only=True)["net"]
    sharp = orc.weight_family(base, "sharp")
    teacher = Renderer(_net(Network, sharp, train=False))
    teacher.device = torch.device("cpu")
    rec = {"amplitude_rel": AMPLITUDE_REL, "stability_draws": STABILITY_DRAWS, "seed": SEED, "grad_stride": GRAD_STRIDE}
    rec.update(case(Network, Renderer, "trained_t002", trained, teacher, 0.02, SEED))
    rec.update(case(Network, Renderer, "sharp_t025", sharp, teacher, 0.25, SEED + 1))
    rec.update(case(Network, Renderer, "trained_t025", trained, teacher, 0.25, SEED + 2))
    rec.update(case(Network, Renderer, "coarse_only", trained, teacher, None, SEED + 3, coarse_only=True))
    gg.npz("masked_train.npz", **rec)
    print("bytes:", os.path.getsize(os.path.join(gg.OUT, "masked_train.npz")))


if __name__ == "__main__":
    main()
