"""CPU checks of the deterministic hash-grid table gradient: the integer restatement
(tests/hashgrid_exact_reference.py) against its own claims -- permutation invariance, the derived error bound against the float64
truth, an accumulator far from overflow --, the device helper of csrc/nerf_fixed_sum.h compiled as plain C++ against the restatement,
the fourth header against its binding table, the two pure-host entries by formula, the host refusals of the new entry through the C ABI
and the Python refusals that happen before the library is reached."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import hashgrid_exact_reference as X
import hashgrid_reference as R
from conftest import REPO
from test_fused_mlp_cpu import _declared_signatures, _declared_symbols
from test_gpu_hashgrid import CONFIGS

HEADER = os.path.join(REPO, "include", "nerf_mi355x_hashgrid.h")
NEW_ENTRIES = ("nerf_hashgrid_deterministic_workspace_bytes", "nerf_hashgrid_deterministic_guard_bits",
               "nerf_hashgrid_backward_deterministic")
NAMES = ("default", "dense_then_hashed", "d4_contended", "c1", "c8")
U = 2.0 ** -24


def table(name):
    D, L, C, s, H, T = CONFIGS[name]
    return D, L, C, H, R.level_offsets(D, L, s, H, T), R.level_scales(L, s, H)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_order_independent_accurate_and_cannot_overflow(name):
    D, L, C, H, off, sc = table(name)
    for B in (1, 65, 4096):
        x = R.make_inputs(B, D, H, seed=B)
        go = torch.randn(B, L * C, generator=torch.Generator().manual_seed(B))
        K = X.guard_bits(B, D)
        res = X.exact_table_gradient(x, off, sc, go, C, K)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(1))
        again = X.exact_table_gradient(x[perm], off, sc, go[perm], C, K)
        assert np.array_equal(res["grad"].numpy().view(np.uint32), again["grad"].numpy().view(np.uint32))
        assert np.array_equal(res["acc"], again["acc"]) and np.array_equal(res["emax"], again["emax"])
        # the bound of the GPU test: term formation + truncation + the one rounding
        t = R.truth_f64(x, torch.zeros(off[-1], C), off, sc, go)
        truth, k = t["grad_emb"].numpy(), t["grad_emb_count"].numpy()
        err = np.abs(res["grad"].double().numpy() - truth)
        bound = (2 * D + 2) * U * t["grad_emb_abs"].numpy() + X.truncation_bound(k, res["emax"], K) + U * np.abs(truth)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        print(f"    {name} B={B} K={K}: max err / bound = {ratio:.3f}, log2 max|acc| = {np.log2(max(1, res['max_abs_acc'])):.1f}, "
              f"log2 max sum|q| = {np.log2(max(1.0, res['max_sum_abs_q'])):.1f}, most terms in one element {int(k.max())}")
        assert (err <= bound).all()
        assert res["max_abs_acc"] < 2 ** 63 and res["max_sum_abs_q"] < 2.0 ** 63
        assert k.max() <= B * 2 ** D                                       # what K is sized for
        assert (res["grad"].numpy()[k == 0] == 0).all() and float(res["grad"].abs().max()) > 0


def vertex_case(D, L, C, H):
    """Three identical points on a level-0 cell vertex, grad_out rows 1, 2^-30, -1 in every column."""
    x = torch.full((3, D), float(R.boundary_points(H)[0]))
    go = torch.tensor([1.0, 2.0 ** -30, -1.0])[:, None].expand(3, L * C).contiguous()
    return x, go


def test_restatement_keeps_what_fp32_sums_can_lose():
    """1 + 2^-30 - 1: an fp32 sum in this order gives 0, in another order 2^-30; the exact sum is 2^-30 in every order."""
    D, L, C, H, off, sc = table("dense_then_hashed")
    x, go = vertex_case(D, L, C, H)
    g, f = R.cells(x, sc[0])
    assert float(f.abs().max()) == 0.0                                     # on the vertex: corner 0 weighs exactly 1, the others 0
    row = int(R.corner_rows(g, 0, off[1] - off[0], sc[0])[0])
    assert X.guard_bits(3, D) == 30
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        res = X.exact_table_gradient(x[order], off, sc, go[order], C, 30)
        assert (res["grad"][row] == 2.0 ** -30).all(), order
        assert (res["emax"][row] == 127).all() and (res["acc"][row] == 1 << 23).all()
        level0 = res["grad"][:off[1]].clone()
        level0[row] = 0
        assert float(level0.abs().max()) == 0.0 and (np.delete(res["emax"][:off[1]], row, 0) == 0).all()   # null terms leave no trace


def test_restatement_poison_and_accumulation():
    D, L, C, H, off, sc = table("c1")
    B = 65
    x = R.make_inputs(B, D, H, seed=3)
    go = torch.randn(B, L * C, generator=torch.Generator().manual_seed(4))
    K = X.guard_bits(B, D)
    clean = X.exact_table_gradient(x, off, sc, go, C, K)
    prev = torch.randn(off[-1], C, generator=torch.Generator().manual_seed(5))
    into = X.exact_table_gradient(x, off, sc, go, C, K, prev=prev)
    touched = torch.from_numpy(clean["emax"] > 0)
    assert torch.equal(into["grad"][~touched], prev[~touched]) and torch.equal(into["grad"][touched], (prev + clean["grad"])[touched])
    bad = go.clone()
    bad[7, 1 * C] = float("inf")                                           # level 1, point 7
    res = X.exact_table_gradient(x, off, sc, bad, C, K)
    nan = torch.isnan(res["grad"])
    assert 1 <= int(nan.sum()) <= 2 ** D and (res["emax"][nan.numpy()] == 255).all()
    assert bool((nan[off[1]:off[2]]).any()) and not bool(nan[:off[1]].any()) and not bool(nan[off[2]:].any())
    assert torch.equal(res["grad"][~nan], clean["grad"][~nan])
    assert (res["grad"].numpy().view(np.uint32)[nan.numpy()] == X.QNAN_BITS).all()


# ---- the device helper, as plain C++ -------------------------------------------------------------------------------------------------
def test_device_helper_equals_the_restatement(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++",
                            "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fixed_sum_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(REPO, "tests", "fixed_sum_host.cpp")], check=True)
    rng = np.random.default_rng(0)
    n = 20000
    bits = rng.integers(0, 1 << 32, n, dtype=np.int64)
    e = rng.integers(1, 255, n)                                            # live exponents 1..254
    bits = (bits & ~(0xFF << 23)) | (e << 23)
    gap = np.where(rng.random(n) < 0.5, rng.integers(0, 8, n), rng.integers(0, 64, n))
    emax = np.minimum(e + gap, 254)
    K = rng.integers(4, 31, n)
    # the corners: all-ones and all-zeros significands, shifts of exactly K, K + 23, K + 24
    for j, (mant, s) in enumerate([(0x7FFFFF, 0), (0, 0), (0x7FFFFF, 30), (0x7FFFFF, 53), (0x7FFFFF, 54), (0, 54), (0x7FFFFF, 31)]):
        bits[j], emax[j], K[j] = (j % 2 << 31) | (100 << 23) | mant, 100 + s, 30
    want_q = X.quantize(bits.astype(np.uint32), emax, K)
    acc = rng.integers(-(1 << 62), 1 << 62, n) >> rng.integers(0, 62, n)
    acc[:4] = [0, -1, (1 << 24) + 1, -((1 << 25) + 3)]                     # ties and odd roundings
    f_emax, f_K = rng.integers(1, 255, n), rng.integers(4, 31, n)
    with np.errstate(over="ignore"):                                       # (the largest overflow to Inf, in both)
        want_f = np.ldexp(acc.astype(np.float32), (f_emax - 150 - f_K).astype(np.int32)).astype(np.float32).view(np.uint32)
    counts = [1, 2, 3, 8, 9, 1 << 9, (1 << 9) + 1, 4096 * 16, (1 << 31) - 1, 1 << 35]
    lines = [f"q {b} {m} {k}" for b, m, k in zip(bits, emax, K)] + [f"f {a} {m} {k}" for a, m, k in zip(acc, f_emax, f_K)] + \
            [f"k {c}" for c in counts]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 2 * n + len(counts)
    got_q = np.array([int(v) for v in out[:n]])
    assert np.array_equal(got_q, want_q) and np.abs(want_q).max() <= ((1 << 24) - 1) << 30
    assert int(want_q[2]) == 0x7FFFFF | 0x800000 and int(want_q[3]) == -1 and int(want_q[4]) == 0 and int(want_q[5]) == 0
    got_f = np.array([int(v) for v in out[n:2 * n]], dtype=np.uint32)
    assert np.array_equal(got_f, want_f)
    assert [int(v) for v in out[2 * n:]] == [min(30, 39 - (c - 1).bit_length()) for c in counts]


# ---- the host surface ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_fourth_table():
    import nerf_replication_amd._lib as L
    declared = _declared_signatures(HEADER)
    assert sorted(declared) == _declared_symbols(HEADER) == sorted(L.HASHGRID_EXPORTS) == sorted(NEW_ENTRIES)
    assert tuple(L._HASHGRID_PROTOS) == L.HASHGRID_EXPORTS == tuple(L.HASHGRID_SIGNATURES)
    for name in NEW_ENTRIES:
        assert L.HASHGRID_SIGNATURES[name] == declared[name], name
    assert [L.HASHGRID_SIGNATURES[n][0] for n in NEW_ENTRIES] == ["i64", "i32", "status"]
    assert not set(L.HASHGRID_EXPORTS) & (set(L.EXPORTS) | set(L.NN_EXPORTS) | set(L.FIELD_EXPORTS))
    assert len(L.EXPORTS) == 65 and len(L.NN_EXPORTS) == 11 and len(L.FIELD_EXPORTS) == 4     # the three earlier tables do not move


def test_library_exports_the_new_entries():
    import nerf_replication_amd._lib as L
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert L.load().nerf_nn_abi_version() == 1 and L.load().nerf_abi_version() == 3


def test_pure_host_entries_by_formula():
    import nerf_replication_amd._lib as L
    for rows in (1, 7, 8, 21, 22, 1000, 524288 * 16, 2 ** 31 - 1):
        for C in (1, 2, 4, 8):
            got = L.call("nerf_hashgrid_deterministic_workspace_bytes", rows, C)
            assert got == X.workspace_bytes(rows, C) == -(-12 * rows * C // 256) * 256 and got % 256 == 0 and got >= 12 * rows * C
    for rows, C in ((0, 2), (-1, 2), (2 ** 31, 2), (8, 0), (8, 3), (8, 16)):
        assert L.call("nerf_hashgrid_deterministic_workspace_bytes", rows, C) == -1
    import math
    for D in (2, 3, 4):
        top = (2 ** 31 - 1) // D
        for B in (1, 2, 3, 63, 64, 65, 513, 4096, 2 ** 20, 2 ** 20 + 1, 2 ** 26, top):
            K = L.call("nerf_hashgrid_deterministic_guard_bits", B, D)
            assert K == X.guard_bits(B, D) and 4 <= K <= 30
            if B <= 2 ** 26:                                               # (where float64's log2 is beyond doubt)
                assert K == min(30, 39 - math.ceil(math.log2(B * 2 ** D)))
            assert (2 ** 24 - 1) * 2 ** K * B * 2 ** D < 2 ** 63           # the accumulator cannot overflow
        assert L.call("nerf_hashgrid_deterministic_guard_bits", top + 1, D) == -1
    assert L.call("nerf_hashgrid_deterministic_guard_bits", 3, 3) == 30 and L.call("nerf_hashgrid_deterministic_guard_bits", 2 ** 20, 3) == 16
    for B, D in ((0, 3), (-5, 3), (8, 1), (8, 5)):
        assert L.call("nerf_hashgrid_deterministic_guard_bits", B, D) == -1


def test_entry_refuses_before_any_launch():
    """Host code: the pointers are never followed, so this runs without a GPU."""
    import nerf_replication_amd._lib as L
    lib = L.load()
    D, Lv, C, H, off, sc = table("dense_then_hashed")
    off_c, sc_c = (ctypes.c_int32 * (Lv + 1))(*off), (ctypes.c_float * Lv)(*[float(v) for v in sc])
    need = X.workspace_bytes(off[-1] - off[0], C)
    p = 0x10000

    def call(x=p, go=p, B=4, D=D, C=C, Lv=Lv, off=off_c, sc=sc_c, ge=p, ws=p, nbytes=need):
        rc = lib.nerf_hashgrid_backward_deterministic(x, go, B, D, C, Lv, off, sc, ge, ws, nbytes, None)
        assert "nerf_hashgrid_backward_deterministic" in lib.nerf_last_error().decode()
        return rc
    flat = (ctypes.c_int32 * (Lv + 1))(*([0, 8, 8, 16, 24][:Lv + 1]))
    shifted = (ctypes.c_int32 * (Lv + 1))(*[o + 8 for o in off])           # rows = offsets[L] - offsets[0]: the same size
    B31 = (1 << 31) // (Lv * C)
    unsupported = [call(D=5), call(D=1), call(C=3), call(Lv=0), call(Lv=33)]
    invalid = [call(B=0), call(B=-1), call(B=B31), call(off=None), call(sc=None), call(off=flat),
               call(x=None), call(go=None), call(ge=None), call(ws=None),
               call(go=p + 4), call(ge=p + 2), call(ws=p + 8), call(ws=p + 4)]
    short = [call(nbytes=need - 1), call(nbytes=0), call(nbytes=-1), call(nbytes=12 * (off[-1] - off[0]) * C - 1),
             call(off=shifted, nbytes=need - 256)]
    assert unsupported == [-4] * len(unsupported) and invalid == [-1] * len(invalid) and short == [-2] * len(short)


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_the_library(monkeypatch):
    import nerf_replication_amd as pkg
    from nerf_replication_amd import _lib, hashfield, hashgrid

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", reached)
    x, emb = torch.rand(5, 3), torch.zeros(64, 2)
    off = [0, 32, 64]
    for bad in (1, 0, None, "yes", 1.0, np.True_):
        with pytest.raises(ValueError, match="deterministic"):
            hashgrid.hash_encode(x, emb, off, 2, 4, deterministic=bad)
        with pytest.raises(ValueError, match="deterministic"):
            pkg.HashEncoder(num_levels=2, log2_hashmap_size=8, deterministic=bad)
        with pytest.raises(ValueError, match="deterministic"):
            pkg.TriPlane(num_levels=2, log2_hashmap_size=8, deterministic=bad)
    for flag in (False, True):
        with pytest.raises(_lib.NerfLibraryError):                         # CPU tensors: no fallback, whatever the flag
            hashgrid.hash_encode(x, emb, off, 2, 4, deterministic=flag)
        with pytest.raises(_lib.NerfLibraryError):
            hashgrid.hash_encode(x, emb, off, 2, 4, flag)
    enc = pkg.HashEncoder(num_levels=2, log2_hashmap_size=8)
    assert enc.deterministic is False and pkg.HashEncoder(num_levels=2, log2_hashmap_size=8, deterministic=True).deterministic is True
    det = pkg.HashEncoder(num_levels=2, log2_hashmap_size=8, deterministic=True)
    assert list(det.state_dict()) == list(enc.state_dict()) == ["embeddings"]       # a plain attribute
    enc.deterministic = "on"                                               # ... that is checked where it is used
    with pytest.raises(ValueError, match="deterministic"):
        enc(x, normalize=False)
    tri = pkg.TriPlane(num_levels=2, log2_hashmap_size=8, deterministic=True)
    assert tri.xy_plane.deterministic and tri.yz_plane.deterministic and tri.xz_plane.deterministic
    assert not pkg.TriPlane(num_levels=2, log2_hashmap_size=8).xy_plane.deterministic
    # HashField hands the encoder's flag on
    seen = []

    def spy(inputs, embeddings, offsets, s, H, deterministic=False):
        seen.append(deterministic)
        raise _lib.NerfLibraryError("far enough")
    monkeypatch.setattr(hashfield, "hash_encode", spy)
    for flag in (False, True):
        enc3 = pkg.HashEncoder(input_dim=3, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=12, deterministic=flag)
        field = pkg.HashField([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], encoder=enc3)
        with pytest.raises(_lib.NerfLibraryError):
            field._geo(torch.rand(4, 3))
    assert seen == [False, True]
