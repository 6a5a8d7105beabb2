#!/usr/bin/env python3
"""The measurement behind the bound of tests/test_gpu_hashfield_sampling.py::test_training_moves: five training runs of that test's
case with 32 + 32 samples and perturb (HashRenderer.N_importance, .perturb) and five with the uniform 64-sample table, from the same
initial state on the same rays.  Prints the ten final losses and writes them, with the largest ratio of any importance run to any
uniform run and k = twice that ratio, to profiles/hashfield_sampling.json under "training_k"; the test reads k from there.  Needs an
MI355X and the built library.

    python tools/measure_hashfield_sampling_k.py [--runs 5]
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
import hashfield_sampling_reference as SR  # noqa: E402
import test_gpu_hashfield as T  # noqa: E402
import test_gpu_hashfield_sampling as TS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "measure_hashfield_sampling_k.py needs a GPU"
    ck = torch.load(os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"), weights_only=True)
    sd = {k: ck["net"][k] for k in nerf_oracle.state_dict_keys()}
    amd._lib.load()
    rays = T.training_rays(amd, nerf_oracle, sd)
    sampled = [TS.run_training(amd, rays, 32, 32, True) for _ in range(args.runs)]
    uniform = [TS.run_training(amd, rays, 64, 0, False) for _ in range(args.runs)]
    rec = {"importance_first": [s[0] for s in sampled], "importance_last": [s[-1] for s in sampled],
           "uniform_first": [u[0] for u in uniform], "uniform_last": [u[-1] for u in uniform],
           "what": "final losses of 40 train_step calls, 32 + 32 samples with perturb against the uniform 64-sample table"}
    rec["largest_ratio"] = max(rec["importance_last"]) / min(rec["uniform_last"])
    rec["k"] = 2.0 * rec["largest_ratio"]
    print(json.dumps(rec, indent=1))
    SR.record("training_k", rec)


if __name__ == "__main__":
    main()
