#!/usr/bin/env python3
"""Records which path every mode combination of Renderer.render / Renderer.render_geometry takes, or how it is refused.

    python tools/record_render_modes.py --commit HASH [--out tests/golden/render_modes.json] [--hashes FILE]

_lib.call is wrapped to log the entry name and the scalar arguments of every call into the library.  The two calls are then driven
through the full product of AXES below, 32 rays (the smallest batch at which every path launches whole 32-point tiles) or none, on
the committed synthetic checkpoint with torch.manual_seed(0) in front of every row.  Per row the outcome is either the exception
type with its full message, or the ordered list of entries with their scalars, and whether the training grid's `uses` moved.
Identical outcomes are stored once; `rows` holds one index per row, in the order of itertools.product over AXES.  --hashes also
writes the SHA-256 of the returned tensors' bytes per accepted row (not for committing: a kernel change may move bits).

tests/test_render_modes_cpu.py resolves every row without a GPU, tests/test_gpu_render_modes.py replays them; both import the rows
and the driver from here.  Recording needs an MI355X and the built library.  Developer tool."""
import argparse
import contextlib
import ctypes
import hashlib
import itertools
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "render_modes.json")
BOX = [-2.0, -2.0, -2.0, 2.0, 2.0, 2.0]
LATTICE = (9, 12, 17)
N_RAYS = 32

# name -> values, in the order of the product.  sampling = (task, perturb); grad: "no_grad" on an eval network, "train" = grad enabled
# on a .train() network, "rays" = rays that require grad on an eval network
AXES = (("precision", ("f32", "f32x", "f16", "f16m32")),
        ("sampling", (("test", False), ("train", True), ("train", False))),
        ("fast_sampling", (0, 1)),
        ("N_importance", (128, 0)),
        ("occupancy", (False, True)),
        ("train_occupancy", (False, True)),
        ("grad", ("no_grad", "train", "rays")),
        ("call", ("render", "render_geometry")),
        ("n", (0, N_RAYS)))


def rows(precisions=None):
    """Every row as a dict, with its index in the fixture's `rows`."""
    names = [a for a, _ in AXES]
    for i, values in enumerate(itertools.product(*(v for _, v in AXES))):
        row = dict(zip(names, values), index=i)
        if precisions is None or row["precision"] in precisions:
            yield row


def configure(renderer, net, row, occupancy, train_occupancy):
    """Put `row`'s modes on the renderer and its network; the grids are what "set" means for the two grid attributes."""
    net.precision = row["precision"]
    net.train() if row["grad"] == "train" else net.eval()
    renderer.task, renderer.perturb = row["sampling"]
    renderer.fast_sampling = bool(row["fast_sampling"])
    renderer.N_importance = row["N_importance"]
    renderer.occupancy = occupancy if row["occupancy"] else None
    renderer.train_occupancy = train_occupancy if row["train_occupancy"] else None


def grad_mode(row):
    return torch.no_grad() if row["grad"] == "no_grad" else torch.enable_grad()


def _scalar(a):
    if a is None or isinstance(a, (bool, int, float, str)):
        return a
    if isinstance(a, ctypes.Array):
        return [round(float(x), 9) if isinstance(x, float) else x for x in a]
    return "T" if isinstance(a, torch.Tensor) else "T[%d]" % len(a)


@contextlib.contextmanager
def logged_calls(pkg, log):
    """_lib.call wrapped for the duration: (name, scalars...) of every call appended to `log`."""
    real = pkg._lib.call

    def call(name, *args):
        log.append([name] + [_scalar(a) for a in args])
        return real(name, *args)

    pkg._lib.call = call
    try:
        yield
    finally:
        pkg._lib.call = real


class Driver:
    """One network, one renderer, the rays and the grids of the recording; run(row) -> (outcome, returned tensors or None)."""

    def __init__(self, pkg):
        self.pkg = pkg
        sd = torch.load(os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"), weights_only=True)["net"]
        self.net = pkg.Network()
        self.net.load_state_dict({k: v for k, v in sd.items() if k in self.net.state_dict()}, strict=True)
        self.net = self.net.cuda().eval()
        self.renderer = pkg.Renderer(self.net)
        gen = torch.Generator().manual_seed(7)
        d = torch.nn.functional.normalize(torch.randn(N_RAYS, 3, generator=gen), dim=-1)
        self.o, self.d = (-4.0 * d + 0.3 * torch.randn(N_RAYS, 3, generator=gen)).cuda(), d.cuda()
        self.grids, self.precision = {}, None

    def _enter(self, precision):
        """Once per precision, outside the log: the weight streams packed, and the grids of the fp32-accurate precisions built (the
        fp16 rows are handed the f32 grids: every one of them is refused before a grid is looked at, or ignores it)."""
        self.net.precision = precision
        with torch.no_grad():
            for model in ("", "fine"):
                self.net.packed(model)
                if self.pkg._lib.fp32_accurate(precision):
                    self.net.packed_bwd(model)
            if self.pkg._lib.fp32_accurate(precision) and precision not in self.grids:
                build = self.pkg.OccupancyGrid.from_network
                self.grids[precision] = (build(self.net, BOX, LATTICE), build(self.net, BOX, LATTICE, models=("fine",)))
        self.precision = precision

    def run(self, row):
        if row["precision"] != self.precision:
            self._enter(row["precision"])
        occupancy, train_occupancy = self.grids[row["precision"] if row["precision"] in self.grids else "f32"]
        configure(self.renderer, self.net, row, occupancy, train_occupancy)
        occupancy.uses = train_occupancy.uses = 0
        o, d = self.o[:row["n"]], self.d[:row["n"]]
        if row["grad"] == "rays":
            o = o.clone().requires_grad_(True)
        batch = {"rays_o": o[None], "rays_d": d[None]}
        log, out = [], None
        torch.manual_seed(0)
        with grad_mode(row), logged_calls(self.pkg, log):
            try:
                out = getattr(self.renderer, row["call"])(batch)
                outcome = {"calls": log}
            except Exception as exc:                                      # a refusal, in Python or in the library
                outcome = {"raises": [type(exc).__name__, str(exc)]}
        outcome["uses_moved"] = bool(occupancy.uses or train_occupancy.uses)
        if out is not None and not isinstance(out, dict):
            out = {"rgb": out[0], "depth": out[1]}
        return outcome, out


def record(pkg, precisions=None, with_hashes=False):
    """-> ({row index: outcome}, {row index: {name: sha256}})"""
    driver, outcomes, hashes = Driver(pkg), {}, {}
    for row in rows(precisions):
        outcomes[row["index"]], out = driver.run(row)
        if with_hashes and out is not None:
            torch.cuda.synchronize()
            hashes[row["index"]] = {k: hashlib.sha256(v.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for k, v in out.items()}
    return outcomes, hashes


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose behaviour is recorded")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--hashes", default=None)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import nerf_replication_amd as pkg
    if not torch.cuda.is_available():
        raise SystemExit("record_render_modes.py needs a GPU: the accepted rows launch")
    outcomes, hashes = record(pkg, with_hashes=args.hashes is not None)
    unique, index = [], []
    for i in sorted(outcomes):
        if outcomes[i] not in unique:
            unique.append(outcomes[i])
        index.append(unique.index(outcomes[i]))
    doc = {"commit": args.commit, "recorded": True, "axes": [[a, list(map(list, v)) if a == "sampling" else list(v)] for a, v in AXES],
           "outcomes": unique, "rows": index}
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(
            ' "%s": %s' % (k, json.dumps(v) if k != "outcomes" else "[\n  " + ",\n  ".join(json.dumps(o) for o in v) + "\n ]")
            for k, v in doc.items()) + "\n}\n")
    if args.hashes is not None:
        with open(args.hashes, "w") as f:
            json.dump({str(i): h for i, h in sorted(hashes.items())}, f, indent=0, sort_keys=True)
    refused = sum("raises" in o for o in outcomes.values())
    print(f"{len(outcomes)} rows: {refused} refused, {len(outcomes) - refused} accepted, {len(unique)} distinct outcomes -> {args.out}")


if __name__ == "__main__":
    main()
