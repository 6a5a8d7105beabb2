"""Unit orders of the fp32 render MLP on the CPU: the matching's restatement and its properties, the
library's matching as a stand-alone program (plain and under AddressSanitizer / UBSan) against the restatement, the gain of the
statistic plus matching on the CPU oracle, and the host surface (the sixth header and its binding table)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import unit_order_reference as U
from conftest import REPO
from test_fused_mlp_cpu import _declared_signatures, _declared_symbols

sys.path.insert(0, os.path.join(REPO, "tools"))
import dead_ksteps as dk  # noqa: E402

HEADER = os.path.join(REPO, "include", "nerf_mi355x_order.h")
NEW_ENTRIES = ("nerf_pack_model_ordered", "nerf_unit_order_stats", "nerf_unit_order_match")


def seeded_counts():
    """int32 [n, 256, 256], symmetric: counts of random unit-off patterns, heavy ties (values 0..2), a wide range, all zero, all equal."""
    rng = np.random.default_rng(0)
    mats = []
    for tiles, p in ((96, 0.4), (32, 0.5), (7, 0.2)):
        off = (rng.random((tiles, 256)) < p * rng.random(256)[None, :] * 2).astype(np.int64)
        mats.append(off.T @ off)
    for top in (3, 2):
        m = rng.integers(0, top, (256, 256))
        mats.append(np.triu(m, 1) + np.triu(m, 1).T)
    m = rng.integers(0, 2 ** 30, (256, 256))                                # a range beyond the counting pass of the host code
    mats.append(np.triu(m, 1) + np.triu(m, 1).T)
    mats.append(np.zeros((256, 256), np.int64))
    mats.append(np.full((256, 256), 17, np.int64))
    return np.stack(mats).astype(np.int32)


def test_restatement_properties():
    counts = seeded_counts()
    for c in counts:
        order = U.match(c)
        assert sorted(order.tolist()) == list(range(256))
        lo = np.array([order[U.act_feat(s >> 4, s & 15, 0)] for s in range(128)])
        hi = np.array([order[U.act_feat(s >> 4, s & 15, 1)] for s in range(128)])
        assert np.all(lo < hi)                                              # the lower unit sits in lane half 0
        score = c[lo, hi]
        assert np.all(np.diff(score) <= 0)                                  # the deadest pairs first
        ties = np.diff(score) == 0
        assert np.all(np.diff(lo)[ties] > 0)
        assert np.array_equal(U.match(np.triu(c, 1)), order)                # only the upper triangle is read
    # nothing but ties (all zero, all equal): the walk takes (0, 1), (2, 3), ...; in the first matrix k-step 0 holds the global maximum
    assert U.match(counts[-2]).tolist()[:1] == [0] and U.match(counts[-1])[U.act_feat(0, 0, 1)] == 1
    first = U.match(counts[0])
    i, j = np.triu_indices(256, 1)
    assert counts[0][first[U.act_feat(0, 0, 0)], first[U.act_feat(0, 0, 1)]] == counts[0][i, j].max()


def _host_compiler():
    return next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++",
                             "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_host_program_equals_the_restatement(tmp_path, sanitize):
    """tests/unit_order_host.cpp (its own main around csrc/nerf_unit_order_match.h) on the seeded matrices; the sanitized build runs
    once, as an ordinary executable."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "unit_order_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    built = subprocess.run([cxx, "-std=c++17", "-O1", *flags, "-o", exe, os.path.join(REPO, "tests", "unit_order_host.cpp")],
                           capture_output=True, text=True)
    if sanitize and built.returncode != 0 and "sanitize" in built.stderr + built.stdout:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert built.returncode == 0, built.stderr
    counts = seeded_counts()
    path = tmp_path / "counts.bin"
    counts.tofile(path)
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(counts)
    for c, line in zip(counts, lines):
        got = [int(v) for v in line.split()]
        assert sorted(got) == list(range(256))
        assert got == U.match(c).tolist()


def _oracle_tiles(oracle, sd, seed, n_rays):
    """{"coarse" / "fine": {h0..h7: [tiles, 32, 256]}}: the CPU oracle's activations on seeded rays of the bench frame."""
    ids = torch.randperm(800 * 800, generator=torch.Generator().manual_seed(seed))[:n_rays]
    o, d = oracle.pinhole_rays(800, 800, oracle.camera_pose(40.0), pixel_ids=ids)
    with torch.no_grad():
        _, _, parts = oracle.render(sd, o[None], d[None], return_parts=True)
    out = {}
    for key, prefix, t in (("coarse", "model", parts["t_coarse"]), ("fine", "model_fine", parts["t_sorted"])):
        out[key] = dk.tile_activations(sd, prefix, oracle.points_on_rays(o, d, t), parts["viewdirs"])[1]
    return out


def test_calibrated_order_doubles_the_dead_ksteps(oracle, family_sd):
    """Statistic plus matching on the CPU oracle, `base` family: orders from 16 rays of seed 1, dead k-step fractions on 64 held-out
    rays of seed 0.  The sum over the layers a launch skips in (fine h0..h7, coarse h0..h6: the coarse launch ends at the sigma
    head, which is not a GEMM) is at least 1.5 x the layout's (measured: 3.23 against 1.65, 2.26 against 0.98), and no layer
    falls below its layout value."""
    sd = family_sd("base")
    cal, held = _oracle_tiles(oracle, sd, 1, 16), _oracle_tiles(oracle, sd, 0, 64)
    for key, layers in (("fine", U.RELU_FED), ("coarse", U.RELU_FED[:7])):
        before = [U.dead_fraction(held[key][h]) for h in layers]
        after = [U.dead_fraction(held[key][h], U.match(U.co_dead_counts(cal[key][h]).numpy())) for h in layers]
        print(key, "layout", [round(v, 3) for v in before], "re-paired", [round(v, 3) for v in after])
        assert sum(after) >= 1.5 * sum(before), (key, sum(before), sum(after))
        assert all(a >= b for a, b in zip(after, before)), (key, before, after)


def test_permuted_state_dict_is_the_same_network(oracle, family_sd):
    """The host permutation the GPU tests pack against: the oracle's raw of the permuted network equals the original's up to the
    order of the sums."""
    sd = family_sd("base")
    perm = U.permute_state_dict(sd, {"model_fine": U.random_orders(3)})
    g = torch.Generator().manual_seed(0)
    pts, dirs = torch.rand(64, 1, 3, generator=g) * 2 - 1, torch.nn.functional.normalize(torch.randn(64, 3, generator=g), dim=-1)
    with torch.no_grad():
        a = oracle.network_forward(sd, pts, dirs, "fine", mlp_dtype=torch.float64)
        b = oracle.network_forward(perm, pts, dirs, "fine", mlp_dtype=torch.float64)
    assert (a - b).abs().max() <= 1e-9 * a.abs().max()
    assert not torch.equal(perm["model_fine.pts_linears.3.weight"], sd["model_fine.pts_linears.3.weight"])
    assert all(torch.equal(perm[k], sd[k]) for k in sd if k.startswith("model."))


# ---- the host surface ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_sixth_table():
    import nerf_replication_amd._lib as L
    declared = _declared_signatures(HEADER)
    assert sorted(declared) == _declared_symbols(HEADER) == sorted(L.ORDER_EXPORTS) == sorted(NEW_ENTRIES)
    assert tuple(L._ORDER_PROTOS) == L.ORDER_EXPORTS == tuple(L.ORDER_SIGNATURES)
    for name in NEW_ENTRIES:
        assert L.ORDER_SIGNATURES[name] == declared[name], name
    # nerf_pack_model's arguments with the order table behind the parameters
    pack = L.SIGNATURES["nerf_pack_model"][1]
    assert L.ORDER_SIGNATURES["nerf_pack_model_ordered"][1] == pack[:1] + ("u8*",) + pack[1:]
    assert not set(L.ORDER_EXPORTS) & (set(L.EXPORTS) | set(L.NN_EXPORTS) | set(L.FIELD_EXPORTS) | set(L.HASHGRID_EXPORTS) |
                                       set(L.NN_EXACT_EXPORTS))
    # the five earlier tables do not move
    assert (len(L.EXPORTS), len(L.NN_EXPORTS), len(L.FIELD_EXPORTS), len(L.HASHGRID_EXPORTS), len(L.NN_EXACT_EXPORTS)) == (65, 11, 4, 3, 3)


def test_library_matching_equals_the_restatement():
    """nerf_unit_order_match is pure host: callable without a GPU, through the package's call()."""
    import ctypes
    import nerf_replication_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    try:
        L.load()
    except OSError:
        pytest.skip("the library's HIP runtime does not load here")
    for c in seeded_counts()[[0, 3, 5, 6]]:
        out = (ctypes.c_int32 * 256)()
        assert L.call("nerf_unit_order_match", (ctypes.c_int32 * 65536).from_buffer(np.ascontiguousarray(c)), out) == 0
        assert list(out) == U.match(c).tolist()
    assert L.call("nerf_unit_order_match", None, (ctypes.c_int32 * 256)()) != 0


def test_tool_prints_the_re_paired_column(capsys):
    res = dk.probe(dk.load_family(os.path.join(REPO, "tests", "golden", "synthetic_ckpt.pth"), "base"), n_rays=16, seed=0,
                   calibrate_rays=16)
    for key in ("coarse", "fine"):
        rows = [r for r in res[key]["rows"] if r["kstep_dead"] is not None]
        assert all(r["kstep_dead_repaired"] is not None and r["mfma_left_repaired"] <= r["mfma"] for r in rows)
        assert sum(r["kstep_dead_repaired"] for r in rows) > sum(r["kstep_dead"] for r in rows)
        assert res[key]["mfma_left_repaired"] < res[key]["mfma_left"]
