#!/usr/bin/env python3
"""Interleaved in-process A/B timing of builds of the fp32 weight-gradient kernels (companion of tools/ab_bench.py /
ab_train.py).

    python tools/ab_wgrad.py "base:" "noatomic:-DNERF_WG_HACK_NOATOMIC=1" ...
    python tools/ab_wgrad.py parent=/path/to/libnerf_mi355x.so head=nerf_replication_amd/libnerf_mi355x.so --json out.json

A spec is `name:flags` (a variant built by ab_bench.ensure) or `name=path` (a library that exists, e.g. one built from another
commit).  Per variant and round: nerf_wgrad on the small shapes of a training step's fine pass and on one 256 x 256 layer
(AB_POINTS points, default 4096 x 192), in the layouts mlp_backward_impl uses, and one nerf_mlp_backward of the fine model on
the same points -- the chain kernel and every weight gradient, the 8-job 256 x 256 launch among them, which no entry reaches
alone.  Each call between its own pair of HIP events.  Developer tool."""
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import ab_bench  # noqa: E402

# name, (ldz, zc0, n_out), (ldh, hc0, n_in), (ldw, wc0), bias
SHAPES = [("rgb_linear 3x128", (4, 0, 3), (128, 0, 128), (128, 0), True),
          ("alpha_linear 1x256", (4, 3, 1), (256, 0, 256), (256, 0), True),
          ("views feature 128x256", (128, 0, 128), (256, 0, 256), (283, 0), True),
          ("views dirs 128x27", (128, 0, 128), (32, 0, 27), (283, 256), False),
          ("PE->256 256x63", (256, 0, 256), (64, 0, 63), (319, 0), True),
          ("layer 256x256", (256, 0, 256), (256, 0, 256), (256, 0), True),
          # the generic kernel, on the hidden layers of the fused small MLPs (nerf_fused_mlp_backward)
          ("generic 128x128", (128, 0, 128), (128, 0, 128), (128, 0), False),
          ("generic 64x64", (64, 0, 64), (64, 0, 64), (64, 0), False)]
BACKWARD = "mlp_backward"


def main():
    argv = sys.argv[1:]
    json_path = argv.pop(argv.index("--json") + 1) if "--json" in argv else None
    argv = [a for a in argv if a != "--json"]
    libs = {}
    for s in argv:
        if "=" in s.split(":", 1)[0]:
            name, path = s.split("=", 1)
            libs[name] = os.path.abspath(path)
        else:
            name, extra = s.split(":", 1)
            libs[name] = ab_bench.ensure(name, extra, force=os.environ.get("AB_BUILD_ONLY") == "1")
    if os.environ.get("AB_BUILD_ONLY") == "1":
        print("built", list(libs))
        return
    import nerf_replication_amd as pkg
    L = pkg._lib
    P = int(os.environ.get("AB_POINTS", str(4096 * 192)))
    S = 192
    assert P % S == 0, "AB_POINTS: whole rays of 192 samples"
    n_rays = P // S
    dev = torch.device("cuda:0")
    st = L.stream_of(dev)
    bufs = {}
    for name, (ldz, zc0, n_out), (ldh, hc0, n_in), (ldw, wc0), bias in SHAPES:
        bufs[name] = (torch.randn(P, ldz, device=dev), torch.randn(P, ldh, device=dev),
                      torch.zeros(n_out, ldw, device=dev), torch.zeros(n_out, device=dev))
    handles = {}
    for name, path in libs.items():
        lib = ctypes.CDLL(path)
        for fn, (res, args) in L._PROTOS.items():
            f = getattr(lib, fn); f.restype, f.argtypes = res, args
        handles[name] = lib
    # the backward's inputs, made once by the first library (packed models and the save buffer have one layout)
    lib0 = next(iter(handles.values()))
    ck = torch.load(os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"), weights_only=True)["net"]
    net = pkg.Network(); net.load_state_dict(ck); net = net.to(dev).eval()
    params = [p.detach().contiguous() for p in net.model_fine.ordered_params()]
    arr = (ctypes.c_void_p * 24)(*[p.data_ptr() for p in params])
    pk = torch.empty(int(lib0.nerf_packed_model_bytes(0)), dtype=torch.uint8, device=dev)
    pk_b = torch.empty(int(lib0.nerf_packed_bwd_bytes(0)), dtype=torch.uint8, device=dev)
    assert lib0.nerf_pack_model(arr, pk.data_ptr(), 0, st) == 0 and lib0.nerf_pack_model_bwd(arr, pk_b.data_ptr(), 0, st) == 0
    g = torch.Generator(device="cpu").manual_seed(0)
    d = torch.randn(n_rays, 3, generator=g); d = (d / d.norm(dim=-1, keepdim=True)).to(dev)
    o = (torch.randn(n_rays, 3, generator=g) * 0.1 + torch.tensor([0., 0., 4.])).to(dev)
    t = torch.sort(torch.rand(n_rays, S, generator=g) * 4 + 2, dim=-1).values.to(dev).contiguous()
    G = torch.randn(n_rays, S, 4, generator=g).to(dev)
    raw = torch.empty(n_rays, S, 4, device=dev)
    save = torch.empty(int(lib0.nerf_train_save_floats(P)), device=dev)
    gsave = torch.empty(int(lib0.nerf_train_grad_floats(P)), device=dev)
    g_t = torch.empty(n_rays, S, device=dev)
    assert lib0.nerf_mlp_forward_rays_save(o.data_ptr(), d.data_ptr(), t.data_ptr(), S, n_rays, S, pk.data_ptr(), raw.data_ptr(),
                                           save.data_ptr(), 0, st) == 0, lib0.nerf_last_error()
    grads = [torch.zeros_like(p) for p in params]
    garr = (ctypes.c_void_p * 24)(*[x.data_ptr() for x in grads])

    names = [s[0] for s in SHAPES] + [BACKWARD]
    times = {k: {n: [] for n in names} for k in handles}
    first = {}
    rounds = int(os.environ.get("AB_ROUNDS", "7"))
    for rnd in range(rounds + 1):
        for vname, lib in handles.items():
            for name in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if name == BACKWARD:
                    for x in grads:
                        x.zero_()
                    e0.record()
                    rc = lib.nerf_mlp_backward(o.data_ptr(), d.data_ptr(), t.data_ptr(), S, n_rays, S, pk_b.data_ptr(), G.data_ptr(),
                                               save.data_ptr(), gsave.data_ptr(), g_t.data_ptr(), garr, 0, st)
                    dw = torch.cat([x.flatten() for x in grads])
                else:
                    _, (ldz, zc0, n_out), (ldh, hc0, n_in), (ldw, wc0), bias = next(s for s in SHAPES if s[0] == name)
                    dz, hin, dw, db = bufs[name]
                    dw.zero_(); db.zero_()
                    e0.record()
                    rc = lib.nerf_wgrad(dz.data_ptr(), ldz, zc0, n_out, hin.data_ptr(), ldh, hc0, n_in, dw.data_ptr(), ldw, wc0,
                                        db.data_ptr() if bias else None, P, st)
                e1.record(); torch.cuda.synchronize()
                assert rc == 0, lib.nerf_last_error()
                if rnd == 0:
                    if name not in first:
                        first[name] = dw.clone()
                    else:
                        err = ((dw - first[name]).abs().max() / first[name].abs().max()).item()
                        print(f"  {vname} / {name}: max rel diff vs first variant = {err:.2e}")
                else:
                    times[vname][name].append(e0.elapsed_time(e1) * 1e3)
    out = {"points": P, "rounds": rounds, "unit": "us", "variants": {}}
    for vname in handles:
        tot = 0.0
        parts = []
        out["variants"][vname] = {}
        for name in names:
            ts = times[vname][name]
            med = statistics.median(ts)
            out["variants"][vname][name] = {"median": med, "min": min(ts), "max": max(ts)}
            if name in [s[0] for s in SHAPES[:5]]:
                tot += med * (2 if name.startswith("PE") else 1)        # two PE -> 256 layers per pass
            parts.append(f"{name.split()[0]} {med:8.1f} ({min(ts):.1f}..{max(ts):.1f})")
        print(f"{vname:>10}: " + "  ".join(parts) + f"   | small layers of a fine pass {tot:7.1f} us")
    if json_path:
        os.makedirs(os.path.dirname(os.path.abspath(json_path)), exist_ok=True)
        with open(json_path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
