"""CPU checks of the hash-grid encoding: the level table, which levels are dense and which hashed, the float64 truth generator of
tests/hashgrid_reference.py against torch autograd, and the module surface of nerf_replication_amd.hashgrid (no GPU call)."""
import os
import re

import numpy as np
import pytest
import torch

import hashgrid_reference as R
from conftest import REPO

DEFAULT = dict(L=16, s=2, H=16, T=19)


# ---- 1. totals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg, total", [
    (dict(D=3, **DEFAULT), 7131216),
    (dict(D=2, **DEFAULT), 5594336),
    (dict(D=3, L=4, s=2, H=15, T=12), 16384),
])
def test_level_table_totals(cfg, total):
    from nerf_replication_amd import hashgrid as hg
    assert R.level_offsets(**cfg)[-1] == total
    enc = hg.HashEncoder(input_dim=cfg["D"], num_levels=cfg["L"], level_dim=2, per_level_scale=cfg["s"], base_resolution=cfg["H"],
                         log2_hashmap_size=cfg["T"])
    assert enc.offsets.dtype == torch.int32 and enc.offsets.tolist() == R.level_offsets(**cfg)
    assert tuple(enc.embeddings.shape) == (total, 2)
    assert float(enc.embeddings.detach().abs().max()) <= 1e-4 and float(enc.embeddings.detach().std()) > 0
    # the scales the product hands to the kernels are the restatement's, bit for bit
    assert [np.float32(v) for v in hg.level_scales(cfg["L"], cfg["s"], cfg["H"])] == R.level_scales(cfg["L"], cfg["s"], cfg["H"])


# ---- 2. dense or hashed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_default_levels_hashed_except_the_wrapped_ones(D):
    off, sc = R.level_offsets(D=D, **DEFAULT), R.level_scales(16, 2, 16)
    hashed = [R.level_strides(off[l + 1] - off[l], sc[l], D)[0] for l in range(16)]
    assert hashed == [True] * 12 + [False, False] + [True, True]
    if D == 3:
        assert off[1] - off[0] == 4912                                   # 17^3 = 4913 rounded down to a multiple of 8: hashed although it would fit
        assert R.level_strides(off[13] - off[12], sc[12], 3) == (False, [1, 65537, 131073], 196609)
    for l in (12, 13):                                                   # wrapped: the final stride is small only modulo 2^32
        n = off[l + 1] - off[l]
        res1 = int(sc[l]) + 2
        assert res1 ** D > 2 ** 32 and R.level_strides(n, sc[l], D)[2] == res1 ** D % 2 ** 32 <= n


def test_base_resolution_15_makes_level_0_dense():
    for D, rows in ((2, 256), (3, 4096)):
        off, sc = R.level_offsets(D=D, L=4, s=2, H=15, T=19), R.level_scales(4, 2, 15)
        assert off[1] == rows
        hashed, strides, final = R.level_strides(rows, sc[0], D)
        assert not hashed and strides == [16 ** d for d in range(D)] and final == rows
    # (D 3, L 4, H 15, T 12): dense, then three hashed levels of one size
    off, sc = R.level_offsets(D=3, L=4, s=2, H=15, T=12), R.level_scales(4, 2, 15)
    assert [off[l + 1] - off[l] for l in range(4)] == [4096] * 4
    assert [R.level_strides(4096, sc[l], 3)[0] for l in range(4)] == [False, True, True, True]


def test_dense_rows_are_the_plain_grid_index():
    """On a dense level the row is g0 + g1 * 16 (+ g2 * 256): every corner of every cell of the 15-cell grid, by hand."""
    off, sc = R.level_offsets(D=2, L=1, s=2, H=15, T=19), R.level_scales(1, 2, 15)
    gx, gy = torch.meshgrid(torch.arange(15), torch.arange(15), indexing="ij")
    g = torch.stack([gx.reshape(-1), gy.reshape(-1)], dim=1)
    for idx in range(4):
        rows = R.corner_rows(g, idx, off[1], sc[0])
        assert torch.equal(rows, (g[:, 0] + (idx & 1)) + (g[:, 1] + (idx >> 1)) * 16)


# ---- 3. the truth generator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D, L, C, s, H, T", [(3, 16, 2, 2, 16, 19), (2, 4, 2, 2, 15, 19), (4, 2, 2, 2, 3, 8), (2, 3, 1, 1.5, 7, 8)])
def test_float64_gradients_agree_with_autograd(D, L, C, s, H, T):
    off, sc = R.level_offsets(D, L, s, H, T), R.level_scales(L, s, H)
    gen = torch.Generator().manual_seed(D * 100 + L)
    x = R.make_inputs(257, D, H, seed=3)
    emb = torch.rand(off[-1], C, generator=gen) * 2 - 1
    go = torch.randn(257, L * C, generator=gen)
    truth = R.truth_f64(x, emb, off, sc, go)
    x64 = x.double().requires_grad_(True)
    emb64 = emb.double().requires_grad_(True)
    out = R.forward_autograd_f64(x, x64, emb64, off, sc)
    gx, ge = torch.autograd.grad(out, (x64, emb64), go.double())
    assert float((out.detach() - truth["out"]).abs().max()) <= 1e-12 * float(truth["out"].abs().max())
    assert float((gx - truth["grad_x"]).abs().max()) <= 1e-12 * float(truth["grad_x"].abs().max())
    assert float((ge - truth["grad_emb"]).abs().max()) <= 1e-12 * float(truth["grad_emb"].abs().max())
    # the fp32 fixed-order forward is that same function to fp32 accuracy (2^D + D + 2 roundings of terms that sum absolutely to <= max|emb|)
    assert float((R.forward_f32(x, emb, off, sc).double() - truth["out"]).abs().max()) <= (2 ** D + 2 * D + 2) * 2.0 ** -24
    # counts: every (point, level, corner) is one term of one row, every (level, channel, half-corner) one term of one input
    assert float(truth["grad_emb_count"].sum()) == 257 * L * C * 2 ** D
    assert bool((truth["grad_x_count"] == L * C * 2 ** (D - 1)).all())
    # the index_add_ baseline computes the same gradients
    be, bx = R.backward_f32(x, emb, off, sc, go)
    assert float((be.double() - truth["grad_emb"]).abs().max()) <= 1e-4 * float(truth["grad_emb"].abs().max())
    assert float((bx.double() - truth["grad_x"]).abs().max()) <= 1e-4 * float(truth["grad_x"].abs().max())


def test_inputs_hold_the_edge_rows():
    for H in (16, 15, 7, 3):
        x = R.make_inputs(64, 3, H, seed=0)
        assert bool((x[0] == 0).all() and (x[1] == 1).all()) and float(x.min()) >= 0 and float(x.max()) <= 1
        _, f = R.cells(x, np.float32(H - 1))
        assert int((f[2:, :2] == 0).sum()) >= 8                          # points exactly on level-0 cell boundaries


# ---- 4. module surface -------------------------------------------------------------------------------------------------------------
def test_module_surface():
    import nerf_replication_amd as pkg
    from nerf_replication_amd import hashgrid as hg
    assert pkg.HashEncoder is hg.HashEncoder and pkg.TriPlane is hg.TriPlane and pkg.hashgrid is hg
    assert {"HashEncoder", "TriPlane"} <= set(pkg.__all__)
    enc = hg.HashEncoder(num_levels=4, log2_hashmap_size=12)
    assert list(enc.state_dict().keys()) == ["embeddings"]
    assert enc.out_dim == enc.output_dim == 8 and enc.input_dim == 3 and enc.level_dim == 2
    assert [n for n, _ in enc.named_parameters()] == ["embeddings"] and not list(enc.buffers())
    # desired_resolution overrides per_level_scale: the last level's resolution is the desired one
    enc = hg.HashEncoder(num_levels=8, base_resolution=16, desired_resolution=2048, per_level_scale=7, log2_hashmap_size=10)
    assert enc.per_level_scale == pytest.approx(2.0, rel=1e-12)
    assert enc.per_level_scale == R.effective_scale(8, 7, 16, 2048)
    assert enc.offsets.tolist() == R.level_offsets(3, 8, enc.per_level_scale, 16, 10)
    tri = hg.TriPlane(num_levels=4, level_dim=4, log2_hashmap_size=10)
    assert tri.out_dim == 3 * 16 and tri.xy_plane.input_dim == tri.yz_plane.input_dim == tri.xz_plane.input_dim == 2
    assert sorted(tri.state_dict().keys()) == ["xy_plane.embeddings", "xz_plane.embeddings", "yz_plane.embeddings"]
    with pytest.raises(ValueError):
        hg.HashEncoder(input_dim=5)
    with pytest.raises(ValueError):
        hg.HashEncoder(level_dim=3)
    with pytest.raises(ValueError):
        hg.HashEncoder(num_levels=33)


def test_cpu_tensors_and_other_dtypes_raise():
    from nerf_replication_amd import hashgrid as hg
    from nerf_replication_amd._lib import NerfLibraryError
    enc = hg.HashEncoder(num_levels=2, log2_hashmap_size=8)
    with pytest.raises(NerfLibraryError):
        enc(torch.rand(5, 3), normalize=False)
    with pytest.raises(NerfLibraryError):
        hg.TriPlane(num_levels=2, log2_hashmap_size=8)(torch.rand(5, 3), torch.tensor([0., 0, 0, 1, 1, 1]))
    with pytest.raises(NotImplementedError):
        enc(torch.rand(5, 3, dtype=torch.float64), normalize=False)
    with pytest.raises(NotImplementedError):
        enc.half()(torch.rand(5, 3).half(), normalize=False)


def test_symbols_in_header_and_exports():
    import nerf_replication_amd._lib as L
    text = open(os.path.join(REPO, "include", "nerf_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("nerf_hashgrid_forward", "nerf_hashgrid_backward"):
        assert name in L.EXPORTS and re.search(r"\b" + name + r"\s*\(", text)
    assert len(L._PROTOS["nerf_hashgrid_forward"][1]) == 10 and len(L._PROTOS["nerf_hashgrid_backward"][1]) == 12
