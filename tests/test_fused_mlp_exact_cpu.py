"""CPU checks of the fused MLP's exact weight and bias gradients: the integer restatement
(tests/fused_mlp_exact_reference.py) against its own claims -- permutation invariance, 1 + 2^-30 - 1, the exponent invariant, poison
and false poison, the emax = 0 rule, the derived error bound against float64 on heavy-tailed, ReLU-sparse data --, the helper of
csrc/nerf_fixed_sum.h compiled as plain C++ against the restatement, the fifth header against its binding table, the two pure-host
entries by formula, the host refusals of the new entry through the C ABI and the Python refusals that happen before the library is
reached."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fused_mlp_exact_reference as X
import hashgrid_exact_reference as HX
from conftest import REPO
from test_fused_mlp_cpu import _declared_signatures, _declared_symbols, _params

HEADER = os.path.join(REPO, "include", "nerf_mi355x_nn_exact.h")
NEW_ENTRIES = ("nerf_fused_mlp_exact_workspace_bytes", "nerf_fused_mlp_exact_guard_bits", "nerf_fused_mlp_backward_exact")
MAX_ROWS = 8388607


def bits(t):
    return t.contiguous().numpy().view(np.uint32)


def heavy_tailed(B, n_out, n_in, seed):
    """Cauchy-distributed dz with ReLU zeros, ReLU-sparse inputs."""
    g = torch.Generator().manual_seed(seed)
    dz = torch.empty(B, n_out).cauchy_(generator=g) * (torch.rand(B, n_out, generator=g) < 0.5)
    inp = torch.relu(torch.randn(B, n_in, generator=g))
    return dz.float(), inp.float()


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_quantize_is_the_hash_grids():
    """The slab quantisation against the numpy function the hash-grid restatement uses, on live terms; dead terms give 0."""
    rng = np.random.default_rng(1)
    n = 50000
    b = rng.integers(0, 1 << 32, n, dtype=np.int64)
    e = rng.integers(1, 255, n)
    b = (b & ~(0xFF << 23)) | (e << 23)
    emax = np.minimum(e + np.where(rng.random(n) < 0.5, rng.integers(0, 8, n), rng.integers(0, 64, n)), 254)
    K = int(rng.integers(16, 31))
    got = X.quantize(torch.from_numpy(b), torch.from_numpy(emax), K).numpy()
    assert np.array_equal(got, HX.quantize(b.astype(np.uint32), emax, K))
    dead = torch.tensor([0, 1 << 31, 0x7F800000, 0xFFC00000, 0x007FFFFF], dtype=torch.int64)
    assert (X.quantize(dead, torch.full((5,), 200), 30) == 0).all()


@pytest.mark.parametrize("B", [1, 33, 4113])
def test_restatement_is_order_independent_accurate_and_cannot_overflow(B):
    n_out, n_in = 24, 40
    dz, inp = heavy_tailed(B, n_out, n_in, seed=B)
    K = X.guard_bits(B)
    res = X.exact_weight_gradient(dz, inp, K)
    bias = X.exact_bias_gradient(dz, K)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1))
    again, bias_again = X.exact_weight_gradient(dz[perm], inp[perm], K), X.exact_bias_gradient(dz[perm], K)
    for a, b in ((res, again), (bias, bias_again)):
        assert np.array_equal(bits(a["grad"]), bits(b["grad"])) and torch.equal(a["acc"], b["acc"]) and torch.equal(a["emax"], b["emax"])
    assert res["invariant"]                                                # no term's exponent exceeds the element's emax
    assert res["max_abs_acc"] < 2 ** 63 and bias["max_abs_acc"] < 2 ** 63 and (2 ** 24 - 1) * 2 ** K * B < 2 ** 63
    truth = dz.double().T @ inp.double()
    bound = X.error_bound(dz, inp, res["emax"], K, truth)
    ratio = float(((res["grad"].double() - truth).abs() / bound.clamp_min(1e-300)).max())
    btruth = dz.double().sum(0)
    bbound = X.error_bound(dz, None, bias["emax"], K, btruth)
    bratio = float(((bias["grad"].double() - btruth).abs() / bbound.clamp_min(1e-300)).max())
    plain = float(((dz.T @ inp).double() - truth).abs().div(bound.clamp_min(1e-300)).max())
    print(f"    B={B} K={K}: weights err / bound = {ratio:.3f}, bias = {bratio:.3f}, an fp32 matrix product = {plain:.3f}, "
          f"log2 max|acc| = {np.log2(max(1, res['max_abs_acc'])):.1f}")
    assert ratio <= 1.0 and bratio <= 1.0
    assert float(res["grad"].abs().max()) > 0 and float(bias["grad"].abs().max()) > 0


def test_restatement_keeps_what_fp32_sums_can_lose():
    """1 + 2^-30 - 1: an fp32 sum in this order gives 0; the exact sum is 2^-30 in every order."""
    assert X.guard_bits(3) == 30
    col = torch.tensor([1.0, 2.0 ** -30, -1.0])
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0], [1, 0, 2]):
        dz = col[order][:, None].expand(3, 2).contiguous()
        inp = torch.ones(3, 3)
        res, bias = X.exact_weight_gradient(dz, inp, 30), X.exact_bias_gradient(dz, 30)
        assert (res["grad"] == 2.0 ** -30).all() and (bias["grad"] == 2.0 ** -30).all(), order
        assert (res["emax"] == 127).all() and (res["acc"] == 1 << 23).all() and (bias["acc"] == 1 << 23).all()


def test_restatement_poison_false_poison_and_the_emax_zero_rule():
    B, n_out, n_in = 65, 6, 5
    dz, inp = heavy_tailed(B, n_out, n_in, seed=7)
    inp[:, 4] = 0.0                                                        # a dead input column: emax = 0 for column 4
    dz[:, 5] = 2.0 ** -140                                                 # a subnormal dz column: null bias terms, emax = 0
    K = X.guard_bits(B)
    prev = torch.randn(n_out, n_in, generator=torch.Generator().manual_seed(5))
    clean = X.exact_weight_gradient(dz, inp, K)
    into = X.exact_weight_gradient(dz, inp, K, prev=prev)
    assert (clean["emax"][:, 4] == 0).all() and (clean["emax"][:5, :4] > 0).all()
    assert torch.equal(into["grad"][:, 4], prev[:, 4])                     # emax = 0: neither read nor written
    assert np.array_equal(bits(into["grad"][:5, :4]), bits((prev + clean["grad"])[:5, :4]))
    bprev = torch.randn(n_out, generator=torch.Generator().manual_seed(6))
    binto = X.exact_bias_gradient(dz, K, prev=bprev)
    assert int(binto["emax"][5]) == 0 and float(binto["grad"][5]) == float(bprev[5])
    # poison: one Inf in dz poisons its whole row of the weight gradient (where the input column is not dead: Inf * 0 is poison
    # too) and its bias element, and nothing else
    bad = dz.clone()
    bad[7, 2] = float("inf")
    res, bres = X.exact_weight_gradient(bad, inp, K), X.exact_bias_gradient(bad, K)
    nan = torch.isnan(res["grad"])
    assert nan[2].all() and int(nan.sum()) == n_in and (res["emax"][2] == 255).all()
    assert (bits(res["grad"])[nan.numpy()] == X.QNAN_BITS).all()
    assert np.array_equal(bits(res["grad"][~nan]), bits(clean["grad"][~nan]))
    assert torch.isnan(bres["grad"][2]) and int(torch.isnan(bres["grad"]).sum()) == 1
    # a NaN outranks Inf in the column maximum
    bad[9, 2] = float("nan")
    assert int(X.column_max(bad)[2]) > 0x7F800000
    # false poison: no term overflows, the column maxima multiply to 2^128
    dz2, inp2 = torch.zeros(2, 1), torch.zeros(2, 1)
    dz2[0, 0], inp2[0, 0] = 2.0 ** 100, 1.0
    dz2[1, 0], inp2[1, 0] = 1.0, 2.0 ** 28
    res2 = X.exact_weight_gradient(dz2, inp2, 30)
    assert int(res2["emax"][0, 0]) == 255 and bits(res2["grad"])[0, 0] == X.QNAN_BITS
    assert torch.isfinite(dz2 * inp2).all() and float((dz2 * inp2).sum()) == 2.0 ** 100 + 2.0 ** 28
    inp2[1, 0] = 2.0 ** 27                                                 # one binade less: summed
    res3 = X.exact_weight_gradient(dz2, inp2, 30)
    assert int(res3["emax"][0, 0]) == 254 and float(res3["grad"][0, 0]) == 2.0 ** 100


# ---- the device helper, as plain C++ -------------------------------------------------------------------------------------------------
def test_host_program_equals_the_restatement(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++",
                            "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fused_mlp_exact_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-o", exe, os.path.join(REPO, "tests", "fused_mlp_exact_host.cpp")],
                   check=True)
    rng = np.random.default_rng(0)
    n = 20000
    a = rng.integers(0, 1 << 31, n, dtype=np.int64)
    b = rng.integers(0, 1 << 31, n, dtype=np.int64)
    near = rng.random(n) < 0.5                                             # products near the ends of the exponent range
    b[near] = (b[near] & 0x7FFFFF) | (np.clip(254 - (a[near] >> 23) + rng.integers(-3, 4, int(near.sum())), 0, 255) << 23)
    corners = [(0, 0), (0x7F800000, 0), (0x7F800000, 0x3F800000), (0x7FC00000, 0x3F800000), (0x7F7FFFFF, 0x3F800000),
               (0x7F7FFFFF, 0x3F800001), (0x00800000, 0x3F000000), (0x00800000, 0x3F7FFFFF), (0x00FFFFFF, 0x3F000000), (1, 0x7F7FFFFF),
               (0x5F800000, 0x5F800000), (0x5F7FFFFF, 0x5F800000), (0x7F800001, 0)]
    for j, (u, v) in enumerate(corners):
        a[j], b[j] = u, v
    with np.errstate(all="ignore"):
        product = a.astype(np.uint32).view(np.float32) * b.astype(np.uint32).view(np.float32)
    want_p = (product.view(np.uint32).astype(np.int64) >> 23) & 0xFF
    assert np.array_equal(want_p[:64], X.product_exponent(torch.from_numpy(a[:64]), torch.from_numpy(b[:64])).diagonal().numpy())
    assert list(want_p[:13]) == [0, 255, 255, 255, 254, 255, 0, 1, 1, 105, 255, 254, 255]
    # whole elements: heavy-tailed rows, plus the corner elements of the restatement's own tests
    elements = []
    for seed, rows in enumerate((1, 2, 3, 33, 257)):
        dz, inp = heavy_tailed(rows, 4, 4, seed=100 + seed)
        for o in range(4):
            elements.append((X.guard_bits(rows), dz[:, o].clone(), inp[:, o].clone()))
    one = torch.ones(3)
    elements.append((30, torch.tensor([1.0, 2.0 ** -30, -1.0]), one))
    elements.append((30, torch.tensor([2.0 ** 100, 1.0]), torch.tensor([1.0, 2.0 ** 28])))          # false poison
    elements.append((30, torch.tensor([float("inf"), 1.0]), torch.tensor([0.0, 1.0])))
    elements.append((30, torch.tensor([2.0 ** -100, 0.0]), torch.tensor([2.0 ** -40, 5.0])))         # emax = 0
    elements.append((16, torch.tensor([1.5, -2.0 ** -40, 2.0 ** -41]), one))                         # truncation of both signs
    lines = [f"p {u} {v}" for u, v in zip(a, b)]
    for K, dz, inp in elements:
        pairs = " ".join(f"{int(d)} {int(h)}" for d, h in zip(bits(dz), bits(inp)))
        lines.append(f"e {K} {len(dz)} {pairs}")
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert np.array_equal(np.array([int(v) for v in out[:n]]), want_p)
    for (K, dz, inp), line in zip(elements, out[n:]):
        res = X.exact_weight_gradient(dz[:, None], inp[:, None], K)
        assert [int(v) for v in line.split()] == [int(res["emax"][0, 0]), int(res["acc"][0, 0]), int(bits(res["grad"])[0, 0])], (K, dz, inp)
    assert len(out) == n + len(elements) + 1 and out[-1] == ""


# ---- the host surface ------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_fifth_table():
    import nerf_replication_amd._lib as L
    declared = _declared_signatures(HEADER)
    assert sorted(declared) == _declared_symbols(HEADER) == sorted(L.NN_EXACT_EXPORTS) == sorted(NEW_ENTRIES)
    assert tuple(L._NN_EXACT_PROTOS) == L.NN_EXACT_EXPORTS == tuple(L.NN_EXACT_SIGNATURES)
    for name in NEW_ENTRIES:
        assert L.NN_EXACT_SIGNATURES[name] == declared[name], name
    assert [L.NN_EXACT_SIGNATURES[n][0] for n in NEW_ENTRIES] == ["i64", "i32", "status"]
    # nerf_fused_mlp_backward's arguments plus the workspace and its size in front of the stream
    assert L.NN_EXACT_SIGNATURES["nerf_fused_mlp_backward_exact"][1] == \
        L.NN_SIGNATURES["nerf_fused_mlp_backward"][1][:-1] + ("void*", "i64", "stream")
    assert not set(L.NN_EXACT_EXPORTS) & (set(L.EXPORTS) | set(L.NN_EXPORTS) | set(L.FIELD_EXPORTS) | set(L.HASHGRID_EXPORTS))
    # the four earlier tables do not move
    assert (len(L.EXPORTS), len(L.NN_EXPORTS), len(L.FIELD_EXPORTS), len(L.HASHGRID_EXPORTS)) == (65, 11, 4, 3)


def test_library_exports_the_new_entries():
    import nerf_replication_amd._lib as L
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert L.load().nerf_nn_abi_version() == 1 and L.load().nerf_abi_version() == 3


def test_pure_host_entries_by_formula():
    import math
    import nerf_replication_amd._lib as L
    for in_dim in (1, 3, 32, 42, 255, 256):
        for width in (64, 128):
            for n_hidden in (1, 2, 8):
                for out_dim in (1, 3, 16):
                    got = L.call("nerf_fused_mlp_exact_workspace_bytes", in_dim, width, n_hidden, out_dim)
                    acc = in_dim * width + (n_hidden - 1) * width * width + width * out_dim + n_hidden * width + out_dim
                    maxima = in_dim + 2 * n_hidden * width + out_dim
                    assert got == X.workspace_bytes(in_dim, width, n_hidden, out_dim) == -(-(8 * acc + 4 * maxima) // 256) * 256
    assert 1.2e6 < L.call("nerf_fused_mlp_exact_workspace_bytes", 256, 128, 8, 16) < 1.25e6
    for bad in ((0, 64, 1, 1), (257, 64, 1, 1), (32, 96, 1, 1), (32, 64, 0, 1), (32, 64, 9, 1), (32, 64, 1, 0), (32, 64, 1, 17), (-1, 128, 2, 3)):
        assert L.call("nerf_fused_mlp_exact_workspace_bytes", *bad) == -1, bad
    for B in (1, 2, 3, 511, 512, 513, 1024, 4113, 2 ** 20, 2 ** 20 + 1, 2 ** 23 - 1):
        K = L.call("nerf_fused_mlp_exact_guard_bits", B)
        assert K == X.guard_bits(B) == min(30, 39 - math.ceil(math.log2(B))) and 16 <= K <= 30
        assert (2 ** 24 - 1) * 2 ** K * B < 2 ** 63                        # the accumulator cannot overflow
    assert L.call("nerf_fused_mlp_exact_guard_bits", 512) == 30 and L.call("nerf_fused_mlp_exact_guard_bits", 513) == 29
    assert L.call("nerf_fused_mlp_exact_guard_bits", MAX_ROWS) == 16
    for B in (0, -1, MAX_ROWS + 1, 2 ** 40):
        assert L.call("nerf_fused_mlp_exact_guard_bits", B) == -1


def test_entry_refuses_before_any_launch():
    """Host code: the pointers are never followed, so this runs without a GPU."""
    import nerf_replication_amd._lib as L
    lib = L.load()
    p = 0x10000
    in_dim, width, n_hidden, out_dim = 32, 64, 2, 3
    need = X.workspace_bytes(in_dim, width, n_hidden, out_dim)
    ptrs = (ctypes.c_void_p * 3)(p, p, p)
    holes = (ctypes.c_void_p * 3)(p, None, p)
    odd = (ctypes.c_void_p * 3)(p, p + 2, p)

    def call(x=p, out=p, go=p, B=4, in_dim=in_dim, width=width, n_hidden=n_hidden, out_dim=out_dim, act=0, w=ptrs, save=p, gsave=p,
             gw=ptrs, gb=ptrs, gx=p, ws=p, nbytes=need):
        rc = lib.nerf_fused_mlp_backward_exact(x, out, go, B, in_dim, width, n_hidden, out_dim, act, w, save, gsave, gw, gb, gx, ws, nbytes,
                                               None)
        assert "nerf_fused_mlp_backward_exact" in lib.nerf_last_error().decode()
        return rc
    unsupported = [call(width=96), call(n_hidden=0), call(n_hidden=9), call(out_dim=0), call(out_dim=17), call(in_dim=0), call(in_dim=257),
                   call(act=2)]
    invalid = [call(B=0), call(B=-1), call(B=MAX_ROWS + 1), call(x=None), call(go=None), call(w=None), call(save=None), call(gsave=None),
               call(gw=None), call(gb=None), call(out=None, act=1), call(w=holes), call(save=p + 4), call(gsave=p + 8), call(x=p + 2),
               call(gw=odd), call(gb=odd), call(ws=None), call(ws=p + 8), call(ws=p + 4)]
    short = [call(nbytes=need - 1), call(nbytes=0), call(nbytes=-1), call(nbytes=X.workspace_bytes(in_dim, width, 1, out_dim))]
    assert unsupported == [-4] * len(unsupported) and invalid == [-1] * len(invalid) and short == [-2] * len(short)


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_the_library(monkeypatch):
    import nerf_replication_amd as pkg
    from nerf_replication_amd import _lib, hashfield

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", reached)
    x = torch.zeros(5, 32)
    w, b = _params(32, 64, 2, 3)
    box = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    small = dict(input_dim=3, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=12)
    for bad in (1, 0, None, "yes", 1.0, np.True_):
        with pytest.raises(ValueError, match="deterministic"):
            pkg.fused_mlp(x, w, b, deterministic=bad)
        with pytest.raises(ValueError, match="deterministic"):
            pkg.FusedMLP(32, 3, deterministic=bad)
        with pytest.raises(ValueError, match="deterministic"):
            pkg.ImageFitNetwork(deterministic=bad)
        with pytest.raises(ValueError, match="deterministic"):
            pkg.HashField(box, encoder=pkg.HashEncoder(**small), deterministic=bad)
    for flag in (False, True):
        with pytest.raises(_lib.NerfLibraryError):                         # CPU tensors: no fallback, whatever the flag
            pkg.fused_mlp(x, w, b, deterministic=flag)
        with pytest.raises(_lib.NerfLibraryError):
            pkg.fused_mlp(x, w, b, None, flag)
        with pytest.raises(_lib.NerfLibraryError):
            pkg.FusedMLP(32, 3, deterministic=flag)(x)
        with pytest.raises(_lib.NerfLibraryError):
            pkg.ImageFitNetwork(deterministic=flag).render(torch.zeros(7, 2))
    net = pkg.FusedMLP(32, 3)
    det = pkg.FusedMLP(32, 3, deterministic=True)
    assert net.deterministic is False and det.deterministic is True and list(det.state_dict()) == list(net.state_dict())
    net.deterministic = "on"                                               # a plain attribute, checked where it is used
    with pytest.raises(ValueError, match="deterministic"):
        net(x)
    img = pkg.ImageFitNetwork(deterministic=True)
    assert img.deterministic is True and pkg.ImageFitNetwork().deterministic is False
    assert list(img.state_dict()) == list(pkg.ImageFitNetwork().state_dict())
    # HashField: both heads, and the encoder it builds itself; a caller's encoder keeps its own flag
    for flag in (False, True):
        field = pkg.HashField(box, encoder=pkg.HashEncoder(**small), deterministic=flag)
        assert field.sigma_net.deterministic is flag and field.color_net.deterministic is flag and field.encoder.deterministic is False
        field = pkg.HashField(box, encoder=pkg.HashEncoder(deterministic=True, **small), deterministic=flag)
        assert field.encoder.deterministic is True and field.sigma_net.deterministic is flag
    own = pkg.HashField(box, deterministic=True)
    assert own.encoder.deterministic is True and own.sigma_net.deterministic is True
    assert list(own.state_dict()) == list(pkg.HashField(box).state_dict()) and pkg.HashField(box).encoder.deterministic is False
    # _geo and _rgb hand the heads' flags on
    seen = []

    def spy(x, weights, biases, output_activation=None, deterministic=False):
        seen.append(deterministic)
        return torch.zeros(x.shape[0], weights[-1].shape[0])
    monkeypatch.setattr(hashfield, "fused_mlp", spy)
    monkeypatch.setattr(hashfield, "hash_encode", lambda inputs, *a, **k: torch.zeros(inputs.shape[0], 8))
    for flag in (False, True):
        field = pkg.HashField(box, encoder=pkg.HashEncoder(**small), deterministic=flag)
        field._geo(torch.rand(4, 3))
        field._rgb(torch.rand(4, 32))
        field.color_net.deterministic = not flag
        field._rgb(torch.rand(4, 32))
    assert seen == [False, False, True, True, True, False]
