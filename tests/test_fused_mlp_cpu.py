"""CPU checks of the small-network surface: include/nerf_mi355x_nn.h against _lib's second binding table, the size functions, the
module structure of FusedMLP / ImageFitNetwork, the frequency encoding, and the refusals that happen before the library is touched."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from conftest import REPO

NN_HEADER = os.path.join(REPO, "include", "nerf_mi355x_nn.h")
_C_TYPES = {"int32_t": "i32", "uint32_t": "i32", "int64_t": "i64", "float": "f32", "double": "f64", "uint8_t": "u8", "void": "void"}


def _declared_symbols(path):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nerf_[a-z_0-9]+)\s*\(", text)))


def _declared_signatures(path):
    """{name: (return kind, (parameter kinds))} of every declaration in the header, in the vocabulary of _lib.SIGNATURES (the
    parser of tests/test_abi_symbols.py)."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(const\s+char\s*\*|int32_t|int64_t)\s+(nerf_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        kinds = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(?:const\s+)?(\w+)\s*(\[\d*\])?", " ".join(p.split()))
            assert m, (name, p)
            ctype, star, pname, array = m.groups()
            kind = _C_TYPES[ctype] + star + (array or "")
            assert kind != "void", (name, p)
            kinds.append("stream" if (kind, pname) == ("void*", "stream") else kind)
        assert "stream" not in kinds[:-1], name
        ret = "str" if "char" in ret else "i64" if ret == "int64_t" else "status" if kinds[-1:] == ["stream"] else "i32"
        assert name not in out, name
        out[name] = (ret, tuple(kinds))
    return out


def test_public_names_are_lazy():
    import nerf_replication_amd as pkg
    for name in ("fused_mlp", "FusedMLP", "ImageFitNetwork"):
        assert name in pkg.__all__ and name in dir(pkg) and callable(getattr(pkg, name)), name
    # importing the package still imports no sub-module (a fresh interpreter: this one has imported them already)
    code = ("import sys; sys.path.insert(0, %r); import nerf_replication_amd as p; "
            "assert not [m for m in sys.modules if m.startswith('nerf_replication_amd.')], sys.modules.keys(); "
            "assert p.FusedMLP.__module__ == 'nerf_replication_amd.fused_mlp'" % REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_nn_header_declares_the_second_table():
    import nerf_replication_amd._lib as L
    declared = _declared_signatures(NN_HEADER)
    assert sorted(declared) == _declared_symbols(NN_HEADER) == sorted(L.NN_EXPORTS)
    assert tuple(L._NN_PROTOS) == L.NN_EXPORTS == tuple(L.NN_SIGNATURES)
    for name in L.NN_EXPORTS:
        assert L.NN_SIGNATURES[name] == declared[name], name
        assert len(L._NN_PROTOS[name][1]) == len(declared[name][1])
    assert not set(L.NN_EXPORTS) & set(L.EXPORTS)
    assert len(L.EXPORTS) == 65                    # the core table is frozen; the new entries live in the second one
    assert L.NN_SIGNATURES["nerf_fused_mlp_forward"][1][7:9] == ("f32*[]", "f32*[]")
    assert L._NN_PROTOS["nerf_fused_mlp_backward"][1][12] is ctypes.POINTER(ctypes.c_void_p)


def test_library_exports_the_nn_entries():
    import nerf_replication_amd._lib as L
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in L.NN_EXPORTS:
        assert hasattr(lib, name), name
    assert L.load().nerf_nn_abi_version() == 1 and L.load().nerf_abi_version() == 3
    assert L.call("nerf_nn_abi_version") == 1     # call() finds the names of the second table


@pytest.mark.parametrize("B,width,n_hidden,out_dim", [(1, 64, 1, 1), (33, 128, 4, 3), (4096, 64, 8, 16)])
def test_size_functions(B, width, n_hidden, out_dim):
    """save: n_hidden blocks [B, width]; gsave: the same and one [B, out_dim] block behind them; no padding (the header says so)."""
    import nerf_replication_amd._lib as L
    assert L.call("nerf_fused_mlp_save_floats", B, width, n_hidden) == n_hidden * B * width
    assert L.call("nerf_fused_mlp_grad_floats", B, width, n_hidden, out_dim) == n_hidden * B * width + B * out_dim


def test_size_functions_outside_the_domain():
    import nerf_replication_amd._lib as L
    assert L.call("nerf_fused_mlp_save_floats", 33, 96, 4) == -1 and L.call("nerf_fused_mlp_grad_floats", 33, 96, 4, 3) == -1
    for n_hidden in (0, 9):
        assert L.call("nerf_fused_mlp_save_floats", 33, 128, n_hidden) == -1
        assert L.call("nerf_fused_mlp_grad_floats", 33, 128, n_hidden, 3) == -1
    assert L.call("nerf_fused_mlp_grad_floats", 33, 128, 4, 17) == -1
    assert L.call("nerf_fused_mlp_grad_floats", 33, 128, 4, 0) == -1
    assert L.call("nerf_fused_mlp_save_floats", 0, 128, 4) == -1
    assert L.call("nerf_fused_mlp_save_floats", 8388608, 128, 4) == -1 and L.call("nerf_fused_mlp_save_floats", 8388607, 128, 4) > 0


def test_image_fit_network_state_dict():
    import nerf_replication_amd as pkg
    net = pkg.ImageFitNetwork()
    sd = net.state_dict()
    keys = [f"backbone_layer.{i}.{p}" for i in range(4) for p in ("weight", "bias")] + ["output_layer.0.weight", "output_layer.0.bias"]
    assert list(sd.keys()) == keys
    shapes = [[128, 42], [128]] + [[128, 128], [128]] * 3 + [[3, 128], [3]]
    assert [list(sd[k].shape) for k in keys] == shapes
    assert isinstance(net.backbone_layer, nn.ModuleList) and isinstance(net.output_layer, nn.Sequential)
    assert isinstance(net.output_layer[0], nn.Linear) and isinstance(net.output_layer[1], nn.Sigmoid)
    assert net.chunk_size == 16384 and pkg.ImageFitNetwork(chunk_size=256).chunk_size == 256
    assert not isinstance(net.uv_encoder, nn.Module)          # the frequency encoder has no parameters and no keys
    small = pkg.ImageFitNetwork(D=2, W=64)
    assert [list(v.shape) for v in small.state_dict().values()] == [[64, 42], [64], [64, 64], [64], [3, 64], [3]]


def test_image_fit_network_with_hashgrid():
    import nerf_replication_amd as pkg
    enc = {"type": "cuda_hashgrid", "input_dim": 2, "num_levels": 6, "level_dim": 4, "per_level_scale": 1.5, "base_resolution": 8,
           "log2_hashmap_size": 10}
    net = pkg.ImageFitNetwork(uv_encoder=enc)
    keys = list(net.state_dict().keys())
    assert keys[0] == "uv_encoder.embeddings" and keys[1] == "backbone_layer.0.weight" and len(keys) == 11
    assert isinstance(net.uv_encoder, pkg.HashEncoder)
    assert list(net.state_dict()["backbone_layer.0.weight"].shape) == [128, 6 * 4]
    assert enc["type"] == "cuda_hashgrid"                      # the caller's dict is not consumed
    with pytest.raises(NotImplementedError):
        pkg.ImageFitNetwork(uv_encoder={"type": "cuda_triplane"})
    with pytest.raises(ValueError):
        pkg.ImageFitNetwork(W=96)


def test_fused_mlp_module_state_dict():
    import nerf_replication_amd as pkg
    m = pkg.FusedMLP(32, 3)
    assert list(m.state_dict().keys()) == [f"layers.{i}.{p}" for i in range(3) for p in ("weight", "bias")]
    assert [list(v.shape) for v in m.state_dict().values()] == [[64, 32], [64], [64, 64], [64], [3, 64], [3]]
    m = pkg.FusedMLP(42, 16, width=128, n_hidden=4, output_activation="sigmoid")
    assert isinstance(m.layers, nn.ModuleList) and all(isinstance(l, nn.Linear) for l in m.layers)
    assert [list(l.weight.shape) for l in m.layers] == [[128, 42]] + [[128, 128]] * 3 + [[16, 128]]
    for bad in (dict(width=96), dict(n_hidden=0), dict(n_hidden=9), dict(output_activation="tanh")):
        with pytest.raises(ValueError):
            pkg.FusedMLP(32, 3, **bad)
    with pytest.raises(ValueError):
        pkg.FusedMLP(32, 17)
    with pytest.raises(ValueError):
        pkg.FusedMLP(257, 3)


def test_frequency_encoding_is_the_references():
    """The input, then sin and cos per frequency 2^0 .. 2^9, bit for bit in fp32 on the CPU."""
    import nerf_replication_amd as pkg
    x = torch.rand(5, 2, generator=torch.Generator().manual_seed(3))
    want = torch.cat([x] + [f(x * float(2 ** k)) for k in range(10) for f in (torch.sin, torch.cos)], -1)
    got = pkg.ImageFitNetwork().uv_encoder(x)
    assert got.shape == (5, 42) and got.dtype == torch.float32 and torch.equal(got, want)
    from nerf_replication_amd.fused_mlp import frequency_encode
    assert torch.equal(frequency_encode(x, 3), want[:, :14])


def _params(in_dim, width, n_hidden, out_dim, dtype=torch.float32):
    shapes = [(width, in_dim)] + [(width, width)] * (n_hidden - 1) + [(out_dim, width)]
    return [torch.zeros(s, dtype=dtype) for s in shapes], [torch.zeros(s[0], dtype=dtype) for s in shapes]


def test_refusals_before_the_library(monkeypatch):
    import nerf_replication_amd as pkg
    from nerf_replication_amd import _lib

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", reached)
    x = torch.zeros(5, 32)
    w, b = _params(32, 64, 2, 3)
    with pytest.raises(_lib.NerfLibraryError):                 # CPU tensors: no fallback
        pkg.fused_mlp(x, w, b)
    with pytest.raises(_lib.NerfLibraryError):
        pkg.FusedMLP(32, 3)(x)
    with pytest.raises(_lib.NerfLibraryError):
        pkg.ImageFitNetwork().render(torch.zeros(7, 2))
    for dtype in (torch.float64, torch.float16):
        w2, b2 = _params(32, 64, 2, 3, dtype)
        with pytest.raises(NotImplementedError):
            pkg.fused_mlp(x.to(dtype), w2, b2)
        with pytest.raises(NotImplementedError):
            pkg.fused_mlp(x.to(dtype), w, b)
    with pytest.raises(ValueError):                            # width 96
        pkg.fused_mlp(x, *_params(32, 96, 2, 3))
    with pytest.raises(ValueError):                            # 9 hidden layers
        pkg.fused_mlp(x, *_params(32, 64, 9, 3))
    with pytest.raises(ValueError):                            # out_dim 17
        pkg.fused_mlp(x, *_params(32, 64, 2, 17))
    with pytest.raises(ValueError):                            # ragged: a hidden layer of another width
        pkg.fused_mlp(x, [w[0], torch.zeros(128, 64), torch.zeros(3, 128)], [b[0], torch.zeros(128), b[2]])
    with pytest.raises(ValueError):                            # ragged: the first layer does not take x
        pkg.fused_mlp(torch.zeros(5, 31), w, b)
    with pytest.raises(ValueError):                            # a bias that does not belong to its weight
        pkg.fused_mlp(x, w, [b[0], torch.zeros(63), b[2]])
    with pytest.raises(ValueError):                            # no hidden layer
        pkg.fused_mlp(x, [torch.zeros(3, 32)], [torch.zeros(3)])
    with pytest.raises(ValueError):
        pkg.fused_mlp(x, w, b, output_activation="tanh")
