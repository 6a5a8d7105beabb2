#!/usr/bin/env python3
"""Checkpoint -> PLY: the density of the fine network on an N^3 grid and its iso-surface as a triangle mesh (what the
reference's src/utils/mesh_utils.py extract_mesh is for).

    python examples/extract_mesh.py --ckpt tests/golden/trained_ckpt.pth --n 256 --out mesh.ply
    python examples/extract_mesh.py --level 32                 # the reference's cfg.level; default: picked from the grid
    python examples/extract_mesh.py --precision f16            # fp16 density (PSNR-level accuracy)
    python examples/extract_mesh.py --normals                  # vertex normals (nx ny nz) from the density gradient: smooth shading
    python examples/extract_mesh.py --keep-largest 1 --colors  # the object alone, without floaters, coloured by the network
    python examples/extract_mesh.py --min-triangles 100        # everything bigger than a crumb
    python examples/extract_mesh.py --hashfield field.pth --normals --colors --keep-largest 1      # a HashField (train_hashfield.py --out)

Needs an MI355X and the built library (python -c "import __graft_entry__ as g; g.build()")."""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import nerf_replication_amd as nerf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=os.path.join(REPO, "tests", "golden", "trained_ckpt.pth"))
    ap.add_argument("--n", type=int, default=256, help="grid points per axis (cfg.resolution of the reference)")
    ap.add_argument("--level", type=float, default=None, help="iso level of the pre-ReLU density; default: midway between the "
                    "grid's median and maximum")
    ap.add_argument("--bbox", type=float, nargs=6, default=[-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], metavar="V", help="min xyz, max xyz")
    ap.add_argument("--precision", default="f32", choices=["f32", "f16", "f32x"])
    ap.add_argument("--normals", action="store_true",
                    help="write unit vertex normals -grad sigma / |grad sigma| (nerf.vertex_normals; f32 / f32x)")
    ap.add_argument("--keep-largest", type=int, default=None, metavar="K",
                    help="keep the K connected components with the most triangles (nerf.filter_components)")
    ap.add_argument("--min-triangles", type=int, default=None, metavar="M", help="keep the connected components with at least M triangles")
    ap.add_argument("--colors", action="store_true",
                    help="write vertex colours (red green blue): the network's colour seen head-on from outside (nerf.vertex_colors; f32 / f32x)")
    ap.add_argument("--hashfield", default=None, metavar="PTH",
                    help="a HashField state dict (examples/train_hashfield.py --out) instead of --ckpt; the box is the field's own "
                         "(--bbox and --precision are not used)")
    ap.add_argument("--levels", type=int, default=16, help="with --hashfield: the encoder's levels, as the field was trained")
    ap.add_argument("--log2-hashmap-size", type=int, default=19, help="with --hashfield: the encoder's table size, as the field was trained")
    ap.add_argument("--out", default="mesh.ply")
    args = ap.parse_args()

    if args.hashfield:
        sys.path.insert(0, os.path.join(REPO, "examples"))
        from refine_hashfield_pose import load_field
        net = load_field(args.hashfield, args.levels, args.log2_hashmap_size).cuda().eval().requires_grad_(False)
        args.bbox, args.precision = None, "hash field"
        level = args.level
        if level is None:
            from nerf_replication_amd.mesh import _query_grid, grid_axes
            grid = _query_grid(net.density, grid_axes(net.bbox, args.n)[0], net.wbounds.device)
            level = 0.5 * (grid.median().item() + grid.max().item())
    else:
        net = nerf.Network()
        nerf.load_network(net, args.ckpt)
        net = net.cuda().eval()
        net.precision = args.precision
        level = args.level
        if level is None:
            grid = nerf.density_grid(net, args.bbox, args.n)
            level = 0.5 * (grid.median().item() + grid.max().item())
    torch.cuda.synchronize(); t0 = time.perf_counter()
    vertices, faces = nerf.extract_mesh(net, level, args.bbox, args.out, args.n, normals=True if args.normals else None,
                                        min_triangles=args.min_triangles, keep_largest=args.keep_largest,
                                        colors=True if args.colors else None)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print("{}^3 grid, {}, level {:.4g}: {} vertices, {} triangles in {:.1f} ms (grid + surface{}{}{} + file)".format(
        args.n, args.precision, level, vertices.shape[0], faces.shape[0], dt * 1e3,
        " + component filter" if args.keep_largest is not None or args.min_triangles is not None else "",
        " + vertex normals" if args.normals else "", " + vertex colours" if args.colors else ""))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
