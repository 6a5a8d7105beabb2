#!/usr/bin/env python3
"""Times the hash-grid encoding (3-D default configuration, B = 2^20 uniformly random points): forward, backward into the table
alone, backward into table and input -- the HIP entries against the torch restatement of tests/hashgrid_reference.py on the same GPU
(gathers and index_add_: what a user would write without the kernels).  Device events around each call, a warm-up of every case,
then alternating rounds (HIP, torch, HIP, torch, ...); the record keeps every sample.  Writes profiles/hashgrid_timing.json.  Needs
an MI355X and the built library.

    python tools/time_hashgrid.py [--log2-batch 20] [--rounds 7] [--inner 10] [--out profiles/hashgrid_timing.json]
    python tools/time_hashgrid.py --deterministic      # the table gradient alone: fp32 atomics against the exact sum

--deterministic times nerf_hashgrid_backward (table gradient only) and nerf_hashgrid_backward_deterministic alternately in one
process under the same protocol and writes profiles/hashgrid_deterministic_timing.json; the other record is left alone.

Bytes are counted from the shapes: every (point, level, corner) gathers one row of C floats (forward, and again for the input
gradient) and adds one row of C floats (table gradient).  The rates are those bytes over the call's time -- whole calls, not
kernel times.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import hashgrid_reference as R  # noqa: E402
from nerf_replication_amd import _lib  # noqa: E402

# MI355X_MICROARCH, global float atomics: the chip-wide rates the table gradient is set beside
ATOMIC_TBPS_CONTIGUOUS = 1.3         # 256 contiguous bytes per wave-instruction
ATOMIC_TBPS_LANE_PER_ROW = 0.08      # 64 lanes in 64 different rows


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-batch", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="HIP calls per timed window (the torch baseline is timed one call at a time)")
    ap.add_argument("--deterministic", action="store_true", help="time the deterministic table gradient against the atomic one")
    ap.add_argument("--out", default=None, help="default: profiles/hashgrid_timing.json (--deterministic: "
                                                "profiles/hashgrid_deterministic_timing.json)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "hashgrid_deterministic_timing.json" if args.deterministic else "hashgrid_timing.json")
    assert torch.cuda.is_available(), "time_hashgrid.py needs a GPU"
    assert args.rounds >= 5
    dev = torch.device("cuda")
    D, L, C, s, H, T = 3, 16, 2, 2, 16, 19
    B = 1 << args.log2_batch
    off, sc = R.level_offsets(D, L, s, H, T), R.level_scales(L, s, H)
    off_c = (ctypes.c_int32 * (L + 1))(*off)
    sc_c = (ctypes.c_float * L)(*[float(v) for v in sc])
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, D, device=dev, generator=gen)
    emb = torch.rand(off[-1], C, device=dev, generator=gen) * 2 - 1
    go = torch.randn(B, L * C, device=dev, generator=gen)
    out = torch.empty(B, L * C, device=dev)
    grad_emb, grad_x = torch.zeros_like(emb), torch.empty_like(x)
    lib, st = _lib.load(), _lib.stream_of(dev)

    def hip_forward():
        _lib.check(lib.nerf_hashgrid_forward(x.data_ptr(), emb.data_ptr(), B, D, C, L, off_c, sc_c, out.data_ptr(), st))

    def hip_backward(want_x):
        grad_emb.zero_()                                           # part of every backward: the entry accumulates
        _lib.check(lib.nerf_hashgrid_backward(x.data_ptr(), emb.data_ptr(), go.data_ptr(), B, D, C, L, off_c, sc_c, grad_emb.data_ptr(),
                                              grad_x.data_ptr() if want_x else None, st))

    if args.deterministic:
        return time_deterministic(args, lib, st, hip_backward, dict(x=x, go=go, grad_emb=grad_emb, B=B, D=D, L=L, C=C, s=s, H=H, T=T,
                                                                     off=off, off_c=off_c, sc_c=sc_c))
    cases = {
        "forward": (hip_forward, lambda: R.forward_f32(x, emb, off, sc)),
        "backward_embeddings": (lambda: hip_backward(False), lambda: R.backward_f32(x, emb, off, sc, go, want_x=False)),
        "backward_both": (lambda: hip_backward(True), lambda: R.backward_f32(x, emb, off, sc, go)),
    }
    # the two sides compute the same thing at this size (and this is the warm-up of every case)
    hip_forward()
    ref = cases["forward"][1]()
    assert torch.equal(out, ref), "HIP forward differs from the restatement"
    hip_backward(True)
    ref_e, ref_x = cases["backward_both"][1]()
    err_e = float((grad_emb - ref_e).abs().max() / ref_e.abs().max())
    err_x = float((grad_x - ref_x).abs().max() / ref_x.abs().max())
    assert err_e < 1e-4 and err_x < 1e-4, (err_e, err_x)
    del ref, ref_e, ref_x
    for hip, base in cases.values():
        hip()
        base()
    torch.cuda.synchronize()

    ms = {name: {"hip": [], "torch": []} for name in cases}
    for _ in range(args.rounds):
        for name, (hip, base) in cases.items():
            ms[name]["hip"].append(timed(hip, args.inner))
            ms[name]["torch"].append(timed(base, 1))
    rows = B * L * (1 << D)                                        # (point, level, corner) triples
    row_bytes = C * 4
    gathered = {"forward": rows * row_bytes, "backward_embeddings": 0, "backward_both": rows * row_bytes}
    atomic = {"forward": 0, "backward_embeddings": rows * row_bytes, "backward_both": rows * row_bytes}
    rec = {"device": torch.cuda.get_device_name(0), "config": {"D": D, "L": L, "C": C, "per_level_scale": s, "base_resolution": H,
                                                                "log2_hashmap_size": T, "table_rows": off[-1]},
           "B": B, "rounds": args.rounds, "hip_calls_per_window": args.inner,
           "timer": "device events around whole calls (backward includes zeroing the table gradient); rounds alternate HIP and torch",
           "baseline": "tests/hashgrid_reference.py forward_f32 / backward_f32 on the same GPU (gathers and index_add_)",
           "agreement": {"forward": "bit-equal", "grad_emb_max_rel": err_e, "grad_x_max_rel": err_x},
           "guide_atomic_TBps": {"contiguous_256B": ATOMIC_TBPS_CONTIGUOUS, "one_lane_per_row": ATOMIC_TBPS_LANE_PER_ROW},
           "cases": {}}
    for name in cases:
        hip_ms, base_ms = statistics.median(ms[name]["hip"]), statistics.median(ms[name]["torch"])
        rec["cases"][name] = {
            "hip_ms": stats(ms[name]["hip"]), "torch_ms": stats(ms[name]["torch"]), "speedup_median": base_ms / hip_ms,
            "gathered_bytes": gathered[name], "atomic_bytes": atomic[name],
            "hip_gathered_TBps": gathered[name] / (hip_ms * 1e-3) / 1e12,
            "hip_atomic_TBps": atomic[name] / (hip_ms * 1e-3) / 1e12,
        }
        print(name, json.dumps(rec["cases"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


def time_deterministic(args, lib, st, hip_backward, a):
    """The table gradient alone: the fp32-atomics entry and the deterministic entry, each call with its zero-fill of grad_emb,
    alternating windows in one process."""
    x, go, grad_emb, B, D, L, C = a["x"], a["go"], a["grad_emb"], a["B"], a["D"], a["L"], a["C"]
    rows = a["off"][-1] - a["off"][0]
    nbytes = int(lib.nerf_hashgrid_deterministic_workspace_bytes(rows, C))
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)

    def atomic():
        hip_backward(False)

    def exact():
        grad_emb.zero_()
        _lib.check(lib.nerf_hashgrid_backward_deterministic(x.data_ptr(), go.data_ptr(), B, D, C, L, a["off_c"], a["sc_c"],
                                                            grad_emb.data_ptr(), workspace.data_ptr(), nbytes, st))
    # agreement (and the warm-up): the exact sum twice gives the same bytes, and the atomic sum lies within its own error of it
    exact()
    first = grad_emb.clone()
    exact()
    assert torch.equal(first.view(torch.int32), grad_emb.view(torch.int32)), "two deterministic calls differ"
    atomic()
    rel = float((grad_emb - first).abs().max() / first.abs().max())
    assert rel < 1e-4, rel
    del first
    for fn in (atomic, exact):
        fn()
    torch.cuda.synchronize()
    ms = {"atomic": [], "deterministic": []}
    for _ in range(args.rounds):
        ms["atomic"].append(timed(atomic, args.inner))
        ms["deterministic"].append(timed(exact, args.inner))
    ratio = statistics.median(ms["deterministic"]) / statistics.median(ms["atomic"])
    rec = {"device": torch.cuda.get_device_name(0),
           "config": {"D": D, "L": L, "C": C, "per_level_scale": a["s"], "base_resolution": a["H"], "log2_hashmap_size": a["T"],
                      "table_rows": a["off"][-1]},
           "B": B, "rounds": args.rounds, "calls_per_window": args.inner,
           "timer": "device events around whole calls (each includes zeroing the table gradient; the deterministic entry also "
                    "zero-fills its workspace); windows alternate atomic, deterministic",
           "guard_bits": int(lib.nerf_hashgrid_deterministic_guard_bits(B, D)), "workspace_bytes": nbytes,
           "agreement": {"deterministic_run_to_run": "bit-equal", "atomic_vs_deterministic_max_rel": rel},
           "atomic_ms": stats(ms["atomic"]), "deterministic_ms": stats(ms["deterministic"]), "ratio_of_medians": ratio}
    print(json.dumps({k: rec[k] for k in ("atomic_ms", "deterministic_ms", "ratio_of_medians")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
