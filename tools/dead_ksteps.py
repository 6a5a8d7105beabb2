#!/usr/bin/env python3
"""CPU probe (torch, no GPU): how many k-steps of the fp32 render MLP multiply zeros tile-wide.

The fp32 inference kernel (csrc/nerf_mlp_f32.hip.inc, gemm_tiles KSKIP) skips the MFMAs of a k-step whose activation register
is zero in all 64 lanes: both features of the pair {act_feat(t, r, 0), act_feat(t, r, 1)} (csrc/nerf_layout.h) are off at all
32 points of the tile.  This tool evaluates the coarse and the fine network of a checkpoint with the oracle on a seeded sample of
rays of the bench frame (800 x 800, camera_pose(40)), cuts the samples of each ray into the kernel's 32-point tiles, and prints
per ReLU-fed GEMM the fraction of dead k-steps and the MFMAs per tile that remain.  That is the prediction a measured A/B of
NERF_DEAD_KSTEP_SKIP is set against, and what corrects bench.py's roofline figures (which count every MFMA as issued).

    python tools/dead_ksteps.py --family base --rays 768

--calibrate-rays N adds the re-paired column: unit orders matched from the co-dead counts of N other rays
(seed + 1) with the library's rule in its restatement (tests/unit_order_reference.py), evaluated on the same tiles as today's.

    python tools/dead_ksteps.py --family base --rays 256 --calibrate-rays 16

--tile-rays R (2, 4, 8, 16, 32) cuts the tiles as the kernel does under NERF_TILE_RAYS=R ("Tile shape"): the
evaluation rays come as seeded runs of R consecutive pixels, and a tile is R neighbouring rays by 32 / R consecutive samples.  The
calibration rays stay scattered and their tiles one-ray, as the library forms unit orders.

    python tools/dead_ksteps.py --family base --rays 512 --calibrate-rays 16 --tile-rays 4
"""
import argparse
import json
import os
import re
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import nerf_oracle as orc            # noqa: E402
from pack_reference import act_feat  # noqa: E402  (the pairing is taken from the layout's statement, not restated)
import unit_order_reference as uor   # noqa: E402  (the matching rule, likewise)

TILE = 32
# Every GEMM of a tile in issue order: (name, k-steps, output tiles, the ReLU output it consumes or None, colour branch?).
# One k-step is one MFMA per output tile.  Training keeps the feature GEMM; the inference instances fold it into the views layer.
GEMMS = (
    ("L0 (PE)", 32, 8, None, False),
    ("L1 (h0)", 128, 8, "h0", False), ("L2 (h1)", 128, 8, "h1", False), ("L3 (h2)", 128, 8, "h2", False),
    ("L4 (h3)", 128, 8, "h3", False),
    ("L5 (PE)", 32, 8, None, False), ("L5 (h4)", 128, 8, "h4", False),
    ("L6 (h5)", 128, 8, "h5", False), ("L7 (h6)", 128, 8, "h6", False),
    ("views, folded (h7)", 128, 4, "h7", True), ("views (dir PE)", 16, 4, None, True),
)


def kstep_pairs():
    """[128, 2]: the two features one activation register holds, k-step s = 16 t + r (register r of input tile t)."""
    return torch.tensor([[act_feat(s >> 4, s & 15, 0), act_feat(s >> 4, s & 15, 1)] for s in range(128)])


def layout_mfmas():
    """(trunk, colour branch) MFMAs of a tile as csrc/nerf_layout.h lays the two weight streams out: every 1-KiB block
    (256 floats) feeds four MFMAs.  Read from the header's own constants."""
    env = {"wsize": lambda ksteps, ntiles: (ksteps // 4) * ntiles * 64 * 4}
    text = open(os.path.join(REPO, "nerf_replication_amd", "csrc", "nerf_layout.h")).read()
    for name, expr in re.findall(r"constexpr\s+int64_t\s+(\w+)\s*=\s*([^;]+);", text):
        try:
            env[name] = eval(expr, {"__builtins__": {}}, env)      # noqa: S307 (the repository's own header)
        except Exception:
            pass                                                   # (expressions with C casts: not needed here)
    return env["kOffFeat"] // 256 * 4, (env["kFoldOffBias"] - env["kFoldOffWvf"]) // 256 * 4


def dead_ksteps(h):
    """h [tiles, 32, 256] post-ReLU activations -> bool [tiles, 128]: the k-step's register is zero at every point."""
    pairs = kstep_pairs()
    off = (h == 0).all(dim=1)                                      # [tiles, 256]: feature off tile-wide
    return off[:, pairs[:, 0]] & off[:, pairs[:, 1]]


def dead_groups(dead):
    """dead bool [tiles, 128] (dead_ksteps) -> (all_dead, leading, runs), int64 [tiles] each, over the 32 four-k-step groups of a
    GEMM: groups whose four k-steps are all dead; the length of the run of such groups the GEMM starts with (the kernel steps
    over it: gemm_tiles, leading dead groups -- but never over the last group, which is counted here all the same); and the
    number of maximal runs of such groups."""
    g = dead.reshape(dead.shape[0], -1, 4).all(dim=-1)                              # [tiles, 32]
    leading = g.long().cumprod(dim=1).sum(dim=1)
    starts = g & ~torch.cat([torch.zeros_like(g[:, :1]), g[:, :-1]], dim=1)
    return g.long().sum(dim=1), leading, starts.long().sum(dim=1)


def stepped_over(leading):
    """The groups the kernel really steps over, from dead_groups' leading run: the last group of a GEMM always runs (it issues
    the next GEMM's prefetch), so a wholly dead input counts 31, not 32.  Trunk GEMMs only: the views GEMM has no group path."""
    return leading.clamp(max=31)


def regroup(x, n, S, tile_rays=1):
    """x [n * S, C], point (ray, sample) at row ray * S + sample -> [n * S / 32, 32, C] in the kernel's tiles: tile T of ray group
    g = T // q (q = S / s, s = 32 / R) holds rays g R .. g R + R - 1 by samples c s .. c s + s - 1 (c = T - g q), lane slot
    j = (ray - g R) s + (sample - c s).  R = 1: 32 consecutive samples of one ray."""
    R, s = tile_rays, TILE // tile_rays
    assert TILE % R == 0 and n % R == 0 and S % s == 0
    return x.reshape(n // R, R, S // s, s, -1).permute(0, 2, 1, 3, 4).reshape(n * S // TILE, TILE, -1)


def tile_activations(sd, prefix, pts, viewdirs, tile_rays=1):
    """pts [n, S, 3] (S a multiple of 32), viewdirs [n, 3] -> (raw [n*S/32, 32, 4], {name: [n*S/32, 32, C]}), fp32 on the CPU."""
    n, S, _ = pts.shape
    assert S % TILE == 0
    emb = torch.cat([orc.freq_encode(pts.reshape(-1, 3), orc.XYZ_FREQS),
                     orc.freq_encode(viewdirs[:, None].expand(n, S, 3).reshape(-1, 3), orc.DIR_FREQS)], -1)
    outs, acts = [], {}
    with torch.no_grad():
        for i in range(0, emb.shape[0], 1 << 15):
            raw, a = orc.nerf_mlp(sd, prefix, emb[i:i + (1 << 15)], return_activations=True)
            outs.append(raw)
            for k, v in a.items():
                acts.setdefault(k, []).append(v)
    tiles = lambda x: regroup(x, n, S, tile_rays)
    return tiles(torch.cat(outs)), {k: tiles(torch.cat(v)) for k, v in acts.items()}


def count(raw, acts, density_only, skip_dead_colour, orders=None):
    """-> per-GEMM rows and totals for a set of tiles.  density_only: the coarse launch (stops after the sigma head);
    skip_dead_colour: tiles without a sigma > 0 skip the colour branch (the fine launch of a render).  orders: {"h0".."h7": order
    [256]} adds the figures of the re-paired network (kstep_dead_repaired, mfma_left_repaired)."""
    n_tiles = raw.shape[0]
    colour = torch.ones(n_tiles, dtype=torch.bool)
    if skip_dead_colour:
        colour = (raw[..., 3] > 0).any(dim=1)
    rows, total, left, left_re = [], 0.0, 0.0, 0.0
    for name, ksteps, ntiles, src, is_colour in GEMMS:
        if is_colour and density_only:
            continue
        runs = colour if is_colour else torch.ones(n_tiles, dtype=torch.bool)
        issued = ksteps * ntiles * runs.float().mean().item()                       # per mean tile, nothing skipped
        frac_dead = frac_off = frac_re = None
        remain = remain_re = issued
        grp = {}                                                                    # per mean tile, over all tiles (as kstep_dead)
        mean_run = lambda x: x.float().mean().item()
        if src is not None:
            dead = dead_ksteps(acts[src])
            grp.update(zip(("groups_dead", "groups_leading", "group_runs"), map(mean_run, dead_groups(dead))))
            grp["groups_stepped"] = 0.0 if is_colour else mean_run(stepped_over(dead_groups(dead)[1]))
            frac_dead = dead.float().mean().item()                                  # over all tiles (the table of the issue)
            frac_off = (acts[src] == 0).all(dim=1).float().mean().item()
            remain = remain_re = ((~dead).float().sum(dim=1) * runs.float()).mean().item() * ntiles
            if orders is not None:
                dead_re = dead_ksteps(acts[src][:, :, torch.as_tensor(orders[src], dtype=torch.long)])
                frac_re = dead_re.float().mean().item()
                remain_re = ((~dead_re).float().sum(dim=1) * runs.float()).mean().item() * ntiles
                grp.update(zip(("groups_dead_repaired", "groups_leading_repaired", "group_runs_repaired"),
                               map(mean_run, dead_groups(dead_re))))
                grp["groups_stepped_repaired"] = 0.0 if is_colour else mean_run(stepped_over(dead_groups(dead_re)[1]))
        rows.append(dict(gemm=name, ksteps=ksteps, ntiles=ntiles, feature_off=frac_off, kstep_dead=frac_dead,
                         mfma=issued, mfma_left=remain, kstep_dead_repaired=frac_re, mfma_left_repaired=remain_re, **grp))
        total += issued
        left += remain
        left_re += remain_re
    return dict(tiles=n_tiles, colour_live=colour.float().mean().item(), rows=rows, mfma=total, mfma_left=left,
                mfma_left_repaired=left_re)


def pixel_runs(n_rays, seed, tile_rays=1, H=800, W=800):
    """Pixel ids of `n_rays` seeded rays: n_rays / R runs of R consecutive pixels of one image row (R = 1: scattered pixels)."""
    R = tile_rays
    assert n_rays % R == 0 and W % R == 0
    starts = torch.randperm(H * W // R, generator=torch.Generator().manual_seed(seed))[:n_rays // R] * R
    return (starts[:, None] + torch.arange(R)).reshape(-1)


def launch_tiles(sd, n_rays, seed, H=800, W=800, theta=40.0, tile_rays=1, run_rays=None):
    """{"coarse" / "fine": (raw, acts)} of the two launches of a render of `n_rays` seeded rays of the bench frame, in tiles of
    `tile_rays` rays (regroup).  The rays are runs of `run_rays` consecutive pixels (default: tile_rays; a multiple of it lets
    two tile shapes be compared on the same rays)."""
    run_rays = tile_rays if run_rays is None else run_rays
    assert run_rays % tile_rays == 0
    ids = pixel_runs(n_rays, seed, run_rays, H, W)
    o, d = orc.pinhole_rays(H, W, orc.camera_pose(theta), pixel_ids=ids)
    with torch.no_grad():
        _, _, parts = orc.render(sd, o[None], d[None], return_parts=True)
    vd = parts["viewdirs"]
    return {key: tile_activations(sd, prefix, orc.points_on_rays(o, d, t), vd, tile_rays)
            for key, prefix, t in (("coarse", "model", parts["t_coarse"]), ("fine", "model_fine", parts["t_sorted"]))}


def probe(sd, n_rays=768, seed=0, H=800, W=800, theta=40.0, calibrate_rays=0, tile_rays=1, run_rays=None):
    """Coarse (64 samples, density only) and fine (192 sorted samples, dead-colour skip) launches of a render of `n_rays` seeded
    rays of the bench frame -> {"coarse": count(...), "fine": count(...)}.  calibrate_rays > 0: with the unit orders matched from
    that many rays of seed + 1, as Renderer.calibrate_unit_order forms them (per model, from its own launch's one-ray tiles).
    tile_rays: the evaluation tiles are that many neighbouring rays by 32 / tile_rays samples (NERF_TILE_RAYS); run_rays as in
    launch_tiles."""
    tiles = launch_tiles(sd, n_rays, seed, H, W, theta, tile_rays, run_rays)
    orders = {"coarse": None, "fine": None}
    if calibrate_rays > 0:
        cal = launch_tiles(sd, calibrate_rays, seed + 1, H, W, theta)
        orders = {key: {h: uor.match(uor.co_dead_counts(cal[key][1][h]).numpy()) for h in uor.RELU_FED} for key in cal}
    return {key: count(*tiles[key], key == "coarse", key == "fine", orders[key]) for key in ("coarse", "fine")}


def load_family(ckpt, family):
    ck = torch.load(ckpt, weights_only=True)
    sd = {k: ck["net"][k] for k in orc.state_dict_keys()}
    return sd if family in ("", "none", "as-is") else orc.weight_family(sd, family)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", default=os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"))
    ap.add_argument("--family", default="base", help="oracle.WEIGHT_FAMILIES name, or 'none' for the checkpoint as stored")
    ap.add_argument("--rays", type=int, default=768)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--calibrate-rays", type=int, default=0, metavar="N",
                    help="also print the re-paired column: unit orders matched from N rays of seed + 1")
    ap.add_argument("--tile-rays", type=int, default=1, choices=(1, 2, 4, 8, 16, 32), metavar="R",
                    help="evaluate on tiles of R neighbouring rays by 32 / R samples (runs of R consecutive pixels)")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    res = probe(load_family(args.ckpt, args.family), args.rays, args.seed, calibrate_rays=args.calibrate_rays,
                tile_rays=args.tile_rays)
    trunk, col = layout_mfmas()
    print(f"{os.path.basename(args.ckpt)} family={args.family} rays={args.rays} seed={args.seed}"
          + (f" tile={args.tile_rays} rays x {TILE // args.tile_rays} samples" if args.tile_rays != 1 else "") + "; "
          f"a full tile issues {trunk} + {col} MFMAs (nerf_layout.h)")
    for key in ("coarse", "fine"):
        r = res[key]
        print(f"\n{key}: {r['tiles']} tiles, colour branch runs in {100 * r['colour_live']:.1f} %")
        re_paired = args.calibrate_rays > 0
        print(f"  {'GEMM':<20} {'feature off':>11} {'k-step dead':>11} {'MFMA/tile':>10} {'left':>10}"
              + (f" {'re-paired':>10} {'left':>10}" if re_paired else ""))
        for row in r["rows"]:
            f = lambda x: "     -" if x is None else f"{x:6.3f}"
            print(f"  {row['gemm']:<20} {f(row['feature_off']):>11} {f(row['kstep_dead']):>11} {row['mfma']:10.1f} {row['mfma_left']:10.1f}"
                  + (f" {f(row['kstep_dead_repaired']):>10} {row['mfma_left_repaired']:10.1f}" if re_paired else ""))
        print(f"  {'total':<20} {'':>11} {'':>11} {r['mfma']:10.1f} {r['mfma_left']:10.1f}"
              + (f" {'':>10} {r['mfma_left_repaired']:10.1f}" if re_paired else "")
              + f"   ({100 * (1 - r['mfma_left'] / r['mfma']):.1f} % skipped"
              + (f", re-paired {100 * (1 - r['mfma_left_repaired'] / r['mfma']):.1f} %)" if re_paired else ")"))
        # all-dead 4-k-step groups (of 32 per GEMM) per mean tile: all of them, those in the GEMM's leading run, number of runs
        # and "stepped": what the kernel steps over -- the leading run without a GEMM's last group, trunk GEMMs only
        print(f"  {'groups (of 32)':<20} {'all dead':>9} {'leading':>9} {'runs':>6} {'stepped':>8}"
              + (f"   {'re-paired:':>10} {'all dead':>9} {'leading':>9} {'runs':>6} {'stepped':>8}" if re_paired else ""))
        tot = [0.0] * 8
        for row in r["rows"]:
            if "groups_dead" not in row:
                continue
            v = [row["groups_dead"], row["groups_leading"], row["group_runs"], row["groups_stepped"]]
            v += [row.get(k + "_repaired", 0.0) for k in ("groups_dead", "groups_leading", "group_runs", "groups_stepped")]
            tot = [a + b for a, b in zip(tot, v)]
            print(f"  {row['gemm']:<20} {v[0]:9.2f} {v[1]:9.2f} {v[2]:6.2f} {v[3]:8.2f}"
                  + (f"   {'':>10} {v[4]:9.2f} {v[5]:9.2f} {v[6]:6.2f} {v[7]:8.2f}" if re_paired else ""))
        print(f"  {'sum':<20} {tot[0]:9.2f} {tot[1]:9.2f} {tot[2]:6.2f} {tot[3]:8.2f}"
              + (f"   {'':>10} {tot[4]:9.2f} {tot[5]:9.2f} {tot[6]:6.2f} {tot[7]:8.2f}" if re_paired else ""))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(ckpt=os.path.basename(args.ckpt), family=args.family, rays=args.rays, seed=args.seed,
                           calibrate_rays=args.calibrate_rays,
                           **({"tile_rays": args.tile_rays} if args.tile_rays != 1 else {}), **res), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
