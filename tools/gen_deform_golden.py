#!/usr/bin/env python3
"""Write tests/golden/deform_delta.npz: the reference's DNeRFNGP.compute_delta in float64 on the CPU, and its autograd gradient of
sum(delta * g) with respect to the three tables.  Data only: inputs, outputs and the gradient.

    python tools/gen_deform_golden.py --reference /path/to/Nerf-Replication [--out tests/golden/deform_delta.npz]

The reference's src/models/encoding/hashencoder/hashgrid.py is imported as it is, under three stubs: `src.config` with a cfg that has
num_frames, an empty `hashencoder.backend` (the CUDA extension is never called by compute_delta), and an object made with
DNeRFNGP.__new__ (HashEncoder.__init__ stops in a debugger) whose `feat` is set by hand.  compute_delta reads F and reso from feat's
shape only, so small tables run the reference's own code.  F = 64, T = 5, R = 8, 257 points: positions that include exactly 0 and
exactly 1, integer and fractional frame numbers."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, T, R, N = 64, 5, 8, 257


def load_reference(root):
    path = os.path.join(root, "src", "models", "encoding", "hashencoder", "hashgrid.py")
    cfg = types.SimpleNamespace(num_frames=T)
    src, config = types.ModuleType("src"), types.ModuleType("src.config")
    config.cfg = cfg
    src.config = config
    package, backend = types.ModuleType("hashencoder"), types.ModuleType("hashencoder.backend")
    package.__path__ = [os.path.dirname(path)]
    backend._backend = None
    sys.modules.update({"src": src, "src.config": config, "hashencoder": package, "hashencoder.backend": backend})
    spec = importlib.util.spec_from_file_location("hashencoder.hashgrid", path)
    module = importlib.util.module_from_spec(spec)
    sys.modules["hashencoder.hashgrid"] = module
    spec.loader.exec_module(module)
    return module


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="root of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "deform_delta.npz"))
    args = ap.parse_args()
    ref = load_reference(args.reference)

    rng = np.random.default_rng(20251)
    # tables of fp32 values (what the kernels hold), scaled so that |delta| reaches a few units; multiples of 1/8, which the
    # archive's compression stores in a fraction of the float64 gradient's bytes (the file stays under 200 KB)
    feat = [(np.round(4.8 * rng.standard_normal((3, F, T, R))) / 8).astype(np.float32) for _ in range(3)]
    # positions on multiples of 2^-8, frame numbers of 2^-4, g of 1/4: every float64 product and sum of the reference is then exact
    # and ends in zero bits, which is what lets 184 KB of float64 gradient fit the archive
    x = (np.floor(rng.random((N, 3)) * 256) / 256).astype(np.float32)
    x[0], x[1], x[2], x[3] = 0.0, 1.0, (0.0, 1.0, 0.5), (1.0, 0.0, 1.0 / 7.0)
    t = (np.floor(rng.random(N) * (T - 1) * 16) / 16).astype(np.float32)
    t[:8] = [0.0, T - 1.0, 1.0, 2.0, 3.0, 0.5, 3.9375, 0.0625]
    t[8:16] = np.arange(8) % T                                              # every integer frame
    g = (np.round(4 * rng.standard_normal((N, 3))) / 4).astype(np.float32)

    model = ref.DNeRFNGP.__new__(ref.DNeRFNGP)
    torch.nn.Module.__init__(model)
    model.feat = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(f).double()) for f in feat])
    delta = model.compute_delta(torch.from_numpy(x).double(), torch.from_numpy(t).double()[:, None])
    (delta * torch.from_numpy(g).double()).sum().backward()
    out = {"x": x, "t": t, "g": g, "delta": delta.detach().numpy()}
    for i in range(3):
        out[f"feat{i}"] = feat[i]
        out[f"grad{i}"] = model.feat[i].grad.numpy()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, max|delta| = {np.abs(out['delta']).max():.3f}")


if __name__ == "__main__":
    main()
