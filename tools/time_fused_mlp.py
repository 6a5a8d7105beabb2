#!/usr/bin/env python3
"""Times the fused MLP (nerf_replication_amd.FusedMLP) against an eager nn.Sequential with the same parameters on the same GPU:
(32 -> 64 x 2 -> 3) and (32 -> 128 x 4 -> 3, sigmoid) at B = 2^16 and 2^20, forward alone (no grad) and forward plus backward with
all gradients (every parameter and x).  Device events around whole calls (module call to the last enqueued kernel, allocations
included), several calls per window, a warm-up of every case, then alternating rounds (fused, eager, fused, eager, ...); the record
keeps every sample.  Then the step time of examples/fit_image.py with and without --fused, alternately, each run a fresh process.
Writes profiles/fused_mlp_timing.json.  Needs an MI355X and the built library.

    python tools/time_fused_mlp.py [--rounds 7] [--inner 10] [--fit-steps 300] [--fit-rounds 3] [--out profiles/fused_mlp_timing.json]
    python tools/time_fused_mlp.py --deterministic [--fit-rounds 9]         # writes profiles/fused_mlp_deterministic_timing.json

--deterministic times the exact, order-independent weight and bias gradients (FusedMLP(deterministic=True))
against the default path, which that mode does not touch: the "train" call of both workloads at both batch sizes, flag off and flag
on alternately in one process under the protocol above, then a 4096-ray HashField training step (192 samples per ray, the default
encoder; table and networks deterministic together) against the default one, and examples/fit_image.py --fused --deterministic
beside the eager MLP for --fit-rounds alternating pairs: the PSNRs, and whether the deterministic runs end with the same parameters.
The other record is left alone.

FLOP are counted from the shapes.  "useful": 2 B n_out n_in per layer (forward), the same again for the transposed products the
backward needs (all layers but the first, plus the first when x wants its gradient) and for the weight gradients.  "executed": what
the MFMAs of the fused kernels issue -- 32-point tiles, reduction and output dimensions padded to multiples of 32 -- so padded tiles
count as executed, and their share is stated.  The fraction of peak is executed FLOP over the call's time over 157.3 TFLOP/s (fp32
MFMA, MI355X) -- whole calls, not kernel times.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import nerf_replication_amd as nerf  # noqa: E402

PEAK_TFLOPS = 157.3
WORKLOADS = {"32-64x2-3": (32, 64, 2, 3, None), "32-128x4-3-sigmoid": (32, 128, 4, 3, "sigmoid")}


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


def pad32(n):
    return (n + 31) // 32 * 32


def flop(B, in_dim, width, n_hidden, out_dim):
    """-> {"forward": (useful, executed), "train": (useful, executed)}; train = forward + gradient chain with grad_x + weight gradients."""
    layers = [(width, in_dim)] + [(width, width)] * (n_hidden - 1) + [(out_dim, width)]
    useful_f = sum(2 * B * o * i for o, i in layers)
    exec_f = sum(2 * pad32(B) * pad32(o) * pad32(i) for o, i in layers)
    return {"forward": (useful_f, exec_f), "train": (3 * useful_f, 3 * exec_f)}


def fit_image_ms(fused, steps):
    cmd = [sys.executable, os.path.join(REPO, "examples", "fit_image.py"), "--steps", str(steps)] + (["--fused"] if fused else [])
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    m = re.search(r"PSNR after \d+ steps: ([\d.]+) dB\s+\(([\d.]+) ms per step", out)
    return float(m.group(2)), float(m.group(1))


def fit_image_run(flags, steps):
    """One fresh-process run of examples/fit_image.py -> (ms per step, PSNR, digest of the final parameters)."""
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "fit_image.py"), "--steps", str(steps)] + flags,
                         capture_output=True, text=True, check=True).stdout
    m = re.search(r"PSNR after \d+ steps: ([\d.]+) dB\s+\(([\d.]+) ms per step", out)
    return float(m.group(2)), float(m.group(1)), re.search(r"parameters sha256: (\w+)", out).group(1)


def deterministic(args):
    """The --deterministic record: flag on against flag off."""
    from nerf_replication_amd.training import FusedAdam, train_step
    dev = torch.device("cuda")
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_window": args.inner,
           "timer": "device events around whole calls (allocations, the workspace and the zeroing of gradients included); rounds "
                    "alternate flag off and flag on in one process",
           "baseline": "the same module with deterministic=False: fp32 atomic sums, the path this mode does not touch",
           "cases": {}}
    for name, (in_dim, width, n_hidden, out_dim, act) in WORKLOADS.items():
        torch.manual_seed(0)
        nets = {False: nerf.FusedMLP(in_dim, out_dim, width, n_hidden, act).to(dev)}
        nets[True] = nerf.FusedMLP(in_dim, out_dim, width, n_hidden, act, deterministic=True).to(dev)
        nets[True].load_state_dict(nets[False].state_dict())
        for log2_b in (16, 20):
            B = 1 << log2_b
            gen = torch.Generator(device=dev).manual_seed(log2_b)
            x = torch.rand(B, in_dim, device=dev, generator=gen).requires_grad_(True)
            go = torch.randn(B, out_dim, device=dev, generator=gen)

            def train(net):
                x.grad = None
                net.zero_grad(set_to_none=True)
                net(x).backward(go)
            grads = {}
            for flag in (False, True):                 # the warm-up of both, and: the two sides compute the same thing
                train(nets[flag])
                grads[flag] = [p.grad.clone() for p in nets[flag].parameters()]
            train(nets[True])
            same = all(torch.equal(a, p.grad) for a, p in zip(grads[True], nets[True].parameters()))
            err = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads[False], grads[True]))
            assert same and err < 1e-3, (same, err)
            torch.cuda.synchronize()
            ms = {False: [], True: []}
            for _ in range(args.rounds):
                for flag in (False, True):
                    ms[flag].append(timed(lambda: train(nets[flag]), args.inner))
            case = {"default_ms": stats(ms[False]), "deterministic_ms": stats(ms[True]),
                    "ratio_median": statistics.median(ms[True]) / statistics.median(ms[False]),
                    "guard_bits": int(nerf._lib.call("nerf_fused_mlp_exact_guard_bits", B)),
                    "workspace_bytes": int(nerf._lib.call("nerf_fused_mlp_exact_workspace_bytes", in_dim, width, n_hidden, out_dim)),
                    "parameter_grad_max_rel_between_the_two": err, "deterministic_run_to_run_equal": same}
            rec["cases"][f"{name}/B=2^{log2_b}/train"] = case
            print(f"{name}/B=2^{log2_b}/train", json.dumps(case), flush=True)
            del x, go
    # a 4096-ray HashField step, the whole field deterministic against the default
    rays = torch.Generator(device=dev).manual_seed(3)
    o = torch.nn.functional.normalize(torch.randn(4096, 3, device=dev, generator=rays), dim=1) * 4.0
    d = torch.nn.functional.normalize(torch.randn(4096, 3, device=dev, generator=rays) * 0.5 - o, dim=1)
    colors = torch.rand(4096, 3, device=dev, generator=rays)
    steps = {}
    for flag in (False, True):
        torch.manual_seed(0)
        field = nerf.HashField((-2.0, -2.0, -2.0, 2.0, 2.0, 2.0), deterministic=flag).to(dev)
        ren = nerf.HashRenderer(field)
        opt = FusedAdam(field.parameters(), lr=1e-2, eps=1e-15, clip_value=40.0)
        steps[flag] = lambda ren=ren, opt=opt: train_step(ren, opt, o, d, colors)
        steps[flag]()
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(args.rounds):
        for flag in (False, True):
            ms[flag].append(timed(steps[flag], args.inner))
    rec["hashfield_step"] = {"rays": 4096, "samples_per_ray": 192, "what": "training.train_step on a default HashField with FusedAdam",
                             "default_ms": stats(ms[False]), "deterministic_ms": stats(ms[True]),
                             "difference_ms_median": statistics.median(ms[True]) - statistics.median(ms[False])}
    print("hashfield_step", json.dumps(rec["hashfield_step"]), flush=True)
    fit = {"eager": [], "deterministic": []}
    for _ in range(args.fit_rounds):
        fit["eager"].append(fit_image_run(["--digest"], args.fit_steps))
        fit["deterministic"].append(fit_image_run(["--fused", "--deterministic"], args.fit_steps))
    rec["fit_image"] = {"steps": args.fit_steps, "pairs": args.fit_rounds, "what": "examples/fit_image.py, a fresh process per run, the eager "
                        "MLP and --fused --deterministic alternately, one seed",
                        "psnr_eager_dB": [r[1] for r in fit["eager"]], "psnr_deterministic_dB": [r[1] for r in fit["deterministic"]],
                        "eager_ms": stats([r[0] for r in fit["eager"]]), "deterministic_ms": stats([r[0] for r in fit["deterministic"]]),
                        "distinct_final_parameters_eager": len({r[2] for r in fit["eager"]}),
                        "distinct_final_parameters_deterministic": len({r[2] for r in fit["deterministic"]})}
    print("fit_image", json.dumps(rec["fit_image"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--fit-steps", type=int, default=300)
    ap.add_argument("--fit-rounds", type=int, default=3)
    ap.add_argument("--deterministic", action="store_true",
                    help="time deterministic=True against the default path instead (writes profiles/fused_mlp_deterministic_timing.json)")
    ap.add_argument("--out", default=None, help="default: profiles/fused_mlp_timing.json (--deterministic: "
                                                "profiles/fused_mlp_deterministic_timing.json)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "fused_mlp_deterministic_timing.json" if args.deterministic else "fused_mlp_timing.json")
    assert torch.cuda.is_available(), "time_fused_mlp.py needs a GPU"
    assert args.rounds >= 5
    if args.deterministic:
        return deterministic(args)
    dev = torch.device("cuda")
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "calls_per_window": args.inner, "peak_fp32_mfma_TFLOPs": PEAK_TFLOPS,
           "timer": "device events around whole module calls (allocations and zeroing of gradients included); rounds alternate fused and eager",
           "baseline": "an eager nn.Sequential (Linear, ReLU, ..., Linear[, Sigmoid]) with the same parameters on the same GPU",
           "cases": {}}
    for name, (in_dim, width, n_hidden, out_dim, act) in WORKLOADS.items():
        torch.manual_seed(0)
        fused = nerf.FusedMLP(in_dim, out_dim, width, n_hidden, act).to(dev)
        mods = [m for l in fused.layers[:-1] for m in (nn.Linear(l.in_features, l.out_features), nn.ReLU())]
        mods.append(nn.Linear(width, out_dim))
        eager = nn.Sequential(*mods, *([nn.Sigmoid()] if act else [])).to(dev)
        with torch.no_grad():
            for dst, src in zip([m for m in eager if isinstance(m, nn.Linear)], fused.layers):
                dst.weight.copy_(src.weight)
                dst.bias.copy_(src.bias)
        for log2_b in (16, 20):
            B = 1 << log2_b
            gen = torch.Generator(device=dev).manual_seed(log2_b)
            x = torch.rand(B, in_dim, device=dev, generator=gen).requires_grad_(True)
            go = torch.randn(B, out_dim, device=dev, generator=gen)

            def forward(net):
                with torch.no_grad():
                    return net(x)

            def train(net):
                x.grad = None
                net.zero_grad(set_to_none=True)
                net(x).backward(go)

            # the two sides compute the same thing (and this is the warm-up of every case)
            err = float((forward(fused) - forward(eager)).abs().max())
            train(fused)
            g_f, gx_f = [p.grad.clone() for p in fused.parameters()], x.grad.clone()
            train(eager)
            g_e, gx_e = [p.grad for p in eager.parameters()], x.grad

            def rel(a, b):
                return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            # among millions of hidden units a few pre-activations lie within rounding of zero, and the two fp32 evaluations may
            # decide their ReLU differently: such a unit moves its own row of grad_x as a whole (recorded, not asserted) and is
            # diluted in the parameter gradients, which sum over all rows
            err_g, err_gx = max(rel(a, b) for a, b in zip(g_f, g_e)), rel(gx_f, gx_e)
            assert err < 1e-4 and err_g < 2e-3, (err, err_g, err_gx)
            torch.cuda.synchronize()
            ms = {c: {"fused": [], "eager": []} for c in ("forward", "train")}
            for _ in range(args.rounds):
                for c, fn in (("forward", forward), ("train", train)):
                    ms[c]["fused"].append(timed(lambda: fn(fused), args.inner))
                    ms[c]["eager"].append(timed(lambda: fn(eager), args.inner))
            counts = flop(B, in_dim, width, n_hidden, out_dim)
            for c in ms:
                f_ms, e_ms = statistics.median(ms[c]["fused"]), statistics.median(ms[c]["eager"])
                useful, executed = counts[c]
                rec["cases"][f"{name}/B=2^{log2_b}/{c}"] = {
                    "fused_ms": stats(ms[c]["fused"]), "eager_ms": stats(ms[c]["eager"]), "speedup_median": e_ms / f_ms,
                    "useful_GFLOP": useful / 1e9, "executed_GFLOP": executed / 1e9, "padded_share_of_executed": 1.0 - useful / executed,
                    "fused_fraction_of_peak_on_executed": executed / (f_ms * 1e-3) / (PEAK_TFLOPS * 1e12),
                    "agreement": {"out_max_abs": err, "parameter_grad_max_rel": err_g, "grad_x_max_rel": err_gx},
                }
                print(f"{name}/B=2^{log2_b}/{c}", json.dumps(rec["cases"][f"{name}/B=2^{log2_b}/{c}"]), flush=True)
            del x, go
    fit = {"fused": [], "eager": [], "psnr_fused": [], "psnr_eager": []}
    for _ in range(args.fit_rounds):
        for key, flag in (("eager", False), ("fused", True)):
            ms_step, db = fit_image_ms(flag, args.fit_steps)
            fit[key].append(ms_step)
            fit["psnr_" + key].append(db)
    rec["fit_image"] = {"steps": args.fit_steps, "batch": 65536, "what": "examples/fit_image.py ms per step (encoder + MLP + Adam), fresh process "
                        "per run, eager and --fused alternately", "eager_ms": stats(fit["eager"]), "fused_ms": stats(fit["fused"]),
                        "psnr_eager_dB": fit["psnr_eager"], "psnr_fused_dB": fit["psnr_fused"]}
    print("fit_image", json.dumps(rec["fit_image"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
