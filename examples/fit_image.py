#!/usr/bin/env python3
"""Fits a 2-D image with the hash-grid encoding: a 2-D HashEncoder (HIP kernels, forward and gradients) feeding a small MLP,
trained with Adam on random pixels of a procedurally generated image (no file input).  Prints the PSNR of the whole image before and
after, and the time per step.  The MLP is eager PyTorch by default (a dozen ATen launches per step); --fused runs the same network,
sigmoid included, through nerf.FusedMLP: one HIP kernel forward, one for the gradient chain.

    python examples/fit_image.py [--size 512] [--steps 1000] [--batch 65536] [--fused] [--width 64] [--hidden 2] [--out fit.ppm]
                                 [--deterministic-table] [--deterministic] [--digest]

--deterministic-table sums the table gradient exactly (HashEncoder(deterministic=True)): the same bytes whatever order the pixels
arrive in, at 1.7 times the time of that kernel.  The MLP's weight gradients keep their fp32 atomics (--fused) or rocBLAS's order.
--deterministic (with --fused) turns on the table and the network together (FusedMLP(deterministic=True)): every gradient of the
step is an exact, order-independent sum, and two runs end with the same parameters, byte for byte -- the last line printed is then a
digest of them (--digest prints it for any run).
"""
import argparse
import hashlib
import math
import os
import sys
import time

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import nerf_replication_amd as nerf  # noqa: E402


def make_image(size, device):
    """[size, size, 3] in [0, 1]: smooth colour ramps, rings that get finer towards one corner, a checkerboard patch and a hard-edged
    disc -- low and high frequencies side by side."""
    v, u = torch.meshgrid(torch.linspace(0, 1, size, device=device), torch.linspace(0, 1, size, device=device), indexing="ij")
    r = torch.sqrt((u - 0.3) ** 2 + (v - 0.35) ** 2)
    rings = 0.5 + 0.5 * torch.cos(2 * math.pi * 40.0 * r * r)
    checker = ((torch.floor(u * 32) + torch.floor(v * 32)) % 2)
    patch = ((u > 0.6) & (v > 0.6)).float()
    disc = (((u - 0.75) ** 2 + (v - 0.25) ** 2) < 0.03).float()
    img = torch.stack([rings * (1 - patch) + checker * patch,
                       (0.2 + 0.6 * u) * (1 - disc) + 0.9 * disc,
                       (0.8 - 0.6 * v) * (1 - disc) + 0.1 * disc], dim=-1)
    return img.clamp(0, 1)


def psnr(a, b):
    return -10.0 * math.log10(float(((a - b) ** 2).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--log2-hashmap-size", type=int, default=15)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--fused", action="store_true", help="run the MLP through nerf.FusedMLP instead of eager torch")
    ap.add_argument("--width", type=int, default=64, help="hidden width (--fused: 64 or 128)")
    ap.add_argument("--hidden", type=int, default=2, help="hidden layers (--fused: 1..8)")
    ap.add_argument("--out", default="", help="write the fitted image as a binary PPM")
    ap.add_argument("--deterministic-table", action="store_true",
                    help="sum the hash table's gradient exactly, in an order-independent way (HashEncoder(deterministic=True))")
    ap.add_argument("--deterministic", action="store_true",
                    help="with --fused: exact, order-independent sums for the table AND the network's weight and bias gradients")
    ap.add_argument("--digest", action="store_true", help="print a SHA-256 of the final parameters (--deterministic does it anyway)")
    args = ap.parse_args()
    if args.deterministic and not args.fused:
        ap.error("--deterministic needs --fused (the eager MLP's weight gradients are rocBLAS's; --deterministic-table alone works with both)")
    assert torch.cuda.is_available(), "fit_image.py needs a GPU"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    img = make_image(args.size, dev)
    v, u = torch.meshgrid(torch.arange(args.size, device=dev), torch.arange(args.size, device=dev), indexing="ij")
    coords = (torch.stack([u, v], dim=-1).float() + 0.5) / args.size              # pixel centres in [0, 1]^2
    enc = nerf.HashEncoder(input_dim=2, num_levels=args.levels, level_dim=2, base_resolution=16,
                           log2_hashmap_size=args.log2_hashmap_size, desired_resolution=args.size,
                           deterministic=args.deterministic_table or args.deterministic).to(dev)
    if args.fused:
        mlp = nerf.FusedMLP(enc.out_dim, 3, width=args.width, n_hidden=args.hidden, output_activation="sigmoid",
                            deterministic=args.deterministic).to(dev)
        network = mlp
    else:
        dims = [enc.out_dim] + [args.width] * args.hidden
        layers = [m for i, o in zip(dims[:-1], dims[1:]) for m in (nn.Linear(i, o), nn.ReLU())]
        mlp = nn.Sequential(*layers, nn.Linear(args.width, 3)).to(dev)

        def network(h):
            return torch.sigmoid(mlp(h))
    opt = torch.optim.Adam([{"params": enc.parameters()}, {"params": mlp.parameters(), "weight_decay": 1e-6}], lr=args.lr,
                           betas=(0.9, 0.99), eps=1e-15)

    def render():
        with torch.no_grad():
            return network(enc(coords, normalize=False))

    print(f"{enc}  table {enc.embeddings.numel() * 4 / 2 ** 20:.1f} MiB, image {args.size}x{args.size}, batch {args.batch}")
    print(f"PSNR before: {psnr(render(), img):.2f} dB")
    gen = torch.Generator(device=dev).manual_seed(1)
    flat_xy, flat_rgb = coords.view(-1, 2), img.view(-1, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(args.steps):
        ids = torch.randint(0, flat_xy.shape[0], (args.batch,), device=dev, generator=gen)
        pred = network(enc(flat_xy[ids], normalize=False))
        loss = ((pred - flat_rgb[ids]) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if (step + 1) % 250 == 0:
            print(f"  step {step + 1}: loss {loss.item():.5f}")
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / max(args.steps, 1) * 1e3
    out = render()
    print(f"PSNR after {args.steps} steps: {psnr(out, img):.2f} dB   ({ms:.2f} ms per step, encoder + {'fused' if args.fused else 'eager'} MLP + Adam)")
    if args.out:
        with open(args.out, "wb") as f:
            f.write(f"P6 {args.size} {args.size} 255\n".encode())
            f.write((out.clamp(0, 1) * 255 + 0.5).to(torch.uint8).cpu().numpy().tobytes())
        print("wrote", args.out)
    if args.deterministic or args.digest:
        digest = hashlib.sha256()
        for p in list(enc.parameters()) + list(mlp.parameters()):
            digest.update(p.detach().cpu().numpy().tobytes())
        print("parameters sha256:", digest.hexdigest())


if __name__ == "__main__":
    main()
