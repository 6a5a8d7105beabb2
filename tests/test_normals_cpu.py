"""CPU checks of the geometry outputs (no GPU): the helpers of tests/normals_reference.py against each other and against closed
forms, the PLY writer with and without vertex normals, and the binding surface of the new C-ABI entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import normals_reference as NR
from conftest import REPO


A_PLANE, C_PLANE = (2.0, -1.0, 4.0), 0.375


@pytest.mark.parametrize("prefix", ["model", "model_fine"])
def test_planar_network_has_the_gradient_a_exactly(synthetic_sd, prefix):
    sd = NR.planar_state_dict(synthetic_sd, A_PLANE, C_PLANE, prefix)
    other = "model" if prefix == "model_fine" else "model_fine"
    assert all(torch.equal(sd[k], synthetic_sd[k]) for k in sd if k.startswith(other + "."))
    assert all(synthetic_sd[k].abs().max() > 0 for k in sd if k.startswith(prefix + ".") and k.endswith("weight"))   # a copy
    pts = (torch.rand(200, 3, generator=torch.Generator().manual_seed(1)) * 6.0 - 3.0)
    a = torch.tensor(A_PLANE)
    for dtype in (torch.float32, torch.float64):
        sigma, g = NR.sigma_and_gradient(sd, prefix, pts, dtype)
        assert sigma.dtype == dtype and g.dtype == dtype
        assert torch.equal(g, a.to(dtype).expand(200, 3))                   # exact: dyadic a, products by +-1 and a/2
        want = pts.double() @ a.double() + C_PLANE
        assert (sigma.double() - want).abs().max() <= (1e-12 if dtype == torch.float64 else 2e-5)   # x + 16 rounds in fp32


def test_fp32_and_fp64_gradients_of_a_real_network_agree(synthetic_sd):
    pts = (torch.rand(64, 3, generator=torch.Generator().manual_seed(2)) * 2.0 - 1.0)
    s32, g32 = NR.sigma_and_gradient(synthetic_sd, "model_fine", pts, torch.float32)
    s64, g64 = NR.sigma_and_gradient(synthetic_sd, "model_fine", pts, torch.float64)
    assert g64.abs().max() > 0
    assert (s32.double() - s64).abs().max() <= 1e-3 * max(1.0, s64.abs().max().item())
    err = (g32.double() - g64).norm(dim=-1) / g64.norm(dim=-1).clamp_min(1e-3 * g64.norm(dim=-1).max())
    assert torch.quantile(err, 0.9) <= 1e-3          # (a ReLU that flips between the two precisions moves single points)


def test_composite_normals_of_a_constant_gradient_ray():
    gen = torch.Generator().manual_seed(3)
    n, S = 5, 50
    raw = torch.randn(n, S, 4, generator=gen)
    raw[..., 3] *= 20.0
    raw[2, :, 3] = -1.0                                                     # an empty ray
    t = torch.linspace(2.0, 6.0, S)[None] + 0.01 * torch.rand(n, S, generator=gen)
    a = torch.tensor(A_PLANE)
    grad = a.expand(n, S, 3).clone()
    normal, acc, w = NR.composite_normals(raw, t, grad)
    a_hat = a.double() / a.double().norm()
    assert normal.dtype == torch.float64 and (w >= 0).all() and (acc <= 1 + 1e-12).all()
    assert (normal + acc[:, None] * a_hat).abs().max() <= 1e-14
    assert acc[2] == 0 and (normal[2] == 0).all() and acc[0] > 0.5
    assert (normal.norm(dim=-1) <= acc + 1e-14).all()
    # the weight of a sample with sigma <= 0 is zero, a zero gradient row gives no normal: only the live rows count
    grad[:, ::2] = 0.0
    normal2, acc2, _ = NR.composite_normals(raw, t, grad)
    live = w * (raw[..., 3] > 0) * (grad.abs().sum(-1) > 0)
    assert torch.equal(acc2, acc) and (normal2 + live.sum(-1)[:, None] * a_hat).abs().max() <= 1e-14


def _mesh4():
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.5, 0.0], [0.25, 0.5, -2.0]])
    f = torch.tensor([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], dtype=torch.int32)
    nrm = torch.tensor([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, -1.0, 0.0], [0.0, 0.0, 0.0]])
    return v, f, nrm


def _write_ply_before_normals(path, vertices, faces):
    """The body of mesh.write_ply as it was before it took `normals` (the bytes a mesh without normals must keep)."""
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype="<f4")
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4")
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("write_ply needs vertices [V,3] and faces [T,3]")
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    rec = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    rec["n"], rec["i"] = 3, f
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(rec.tobytes())


def test_write_ply_with_normals_round_trips(tmp_path):
    from nerf_replication_amd.mesh import write_ply
    v, f, nrm = _mesh4()
    path = tmp_path / "n.ply"
    write_ply(path, v, f, normals=nrm)
    names, rows, faces = NR.parse_ply(path.read_bytes())
    assert names == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(rows[:, :3], v.numpy()) and np.array_equal(rows[:, 3:], nrm.numpy())
    assert np.array_equal(faces, f.numpy())
    with pytest.raises(ValueError):
        write_ply(path, v, f, normals=nrm[:3])


def test_write_ply_without_normals_keeps_its_bytes(tmp_path):
    from nerf_replication_amd.mesh import write_ply
    v, f, _ = _mesh4()
    write_ply(tmp_path / "new.ply", v, f)
    write_ply(tmp_path / "none.ply", v, f, None)
    _write_ply_before_normals(tmp_path / "old.ply", v, f)
    old = (tmp_path / "old.ply").read_bytes()
    assert (tmp_path / "new.ply").read_bytes() == old and (tmp_path / "none.ply").read_bytes() == old
    names, rows, faces = NR.parse_ply(old)
    assert names == ["x", "y", "z"] and np.array_equal(rows, v.numpy()) and np.array_equal(faces, f.numpy())


NEW_ENTRIES = ("nerf_density_gradient_point_bytes", "nerf_density_gradient", "nerf_composite_normals")


def test_new_entries_are_declared_bound_and_exported():
    import nerf_replication_amd._lib as L
    text = open(os.path.join(REPO, "include", "nerf_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nerf_[a-z_0-9]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared and name in L.EXPORTS, name
    assert "#define NERF_ABI_VERSION 3" in text                       # (3: the fold moved into the packed fp32 model)
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    lib.nerf_density_gradient_point_bytes.restype = ctypes.c_int64
    lib.nerf_train_save_floats.restype = lib.nerf_train_grad_floats.restype = ctypes.c_int64
    lib.nerf_train_save_floats.argtypes = lib.nerf_train_grad_floats.argtypes = [ctypes.c_int64]
    per_point = lib.nerf_density_gradient_point_bytes()
    # the bytes per point cover TrainSave + TrainGrad + raw + the seed gradient of any block of whole 32-point tiles (each of the
    # four pieces 256-byte aligned), with less than 1 % to spare
    for pts in (32, 64, 192 * 40, 4096 * 192):
        need = 4 * (lib.nerf_train_save_floats(pts) + lib.nerf_train_grad_floats(pts) + 8 * pts) + 4 * 255
        assert need <= per_point * pts, pts
    assert per_point * (1 << 20) <= 1.01 * 4 * (lib.nerf_train_save_floats(1 << 20) + lib.nerf_train_grad_floats(1 << 20) + 8 * (1 << 20))


def test_python_surface_is_exported():
    import inspect
    import nerf_replication_amd as pkg
    assert callable(pkg.vertex_normals) and callable(pkg.density_gradient) and callable(pkg.Renderer.render_geometry)
    assert list(inspect.signature(pkg.write_ply).parameters) == ["path", "vertices", "faces", "normals"]
    assert inspect.signature(pkg.extract_mesh).parameters["normals"].default is None
    assert inspect.signature(pkg.vertex_normals).parameters["model"].default == "fine"
