#!/usr/bin/env python3
"""The measurement behind the bound of tests/test_gpu_deform.py::test_training_moves: five fused (HashRenderer over a dynamic field +
FusedAdam) and five eager-torch training runs of that test's case, from the same initial state on the same rays.  Prints the ten
final losses and writes them, with the largest ratio of any fused to any eager final loss and k = twice that ratio, to
profiles/deform_parity.json under "training_k"; the test reads k there.  Needs an MI355X and the built library.

    python tools/measure_deform_train_k.py [--runs 5]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import nerf_oracle  # noqa: E402
import nerf_replication_amd as amd  # noqa: E402
import test_gpu_deform as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_deform_train_k.py needs a GPU"
    ck = torch.load(os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"), weights_only=True)
    sd = {k: ck["net"][k] for k in nerf_oracle.state_dict_keys()}
    amd._lib.load()
    rays = T.training_rays(amd, nerf_oracle, sd)
    fused = [T.run_fused(amd, rays)[0] for _ in range(args.runs)]
    eager = [T.run_eager(amd, rays) for _ in range(args.runs)]
    rec = {"fused_first": [f[0] for f in fused], "fused_last": [f[-1] for f in fused],
           "eager_first": [e[0] for e in eager], "eager_last": [e[-1] for e in eager]}
    rec["largest_ratio"] = max(rec["fused_last"]) / min(rec["eager_last"])
    rec["k"] = 2.0 * rec["largest_ratio"]
    print(json.dumps(rec, indent=1))
    T.record("training_k", rec)


if __name__ == "__main__":
    main()
