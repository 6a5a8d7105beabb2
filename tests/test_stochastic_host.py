"""Host checks of stochastic sampling (the reference's task == "train" mode): the renderer accepts the mode and draws in the
reference's order; the CPU restatement the GPU tests compare against reproduces the REAL reference bit for bit; the new
entry points are in the header, the binding and the library."""
import ctypes
import os
import sys
import types

import pytest
import torch

import stochastic_common as SC
from conftest import REPO

NEW_SYMBOLS = ("nerf_stratified_samples", "nerf_sample_fine_rays", "nerf_sample_fine_rays_backward",
               "nerf_render_forward_stochastic", "nerf_render_stochastic_workspace_bytes")


def _renderer_with_cfg(monkeypatch, **cfg):
    """The renderer reads the reference's top-level cfg from src.config, as volume_renderer.py:14-24 does."""
    import nerf_replication_amd as pkg
    mod = types.ModuleType("src.config")
    mod.cfg = types.SimpleNamespace(**cfg)
    monkeypatch.setitem(sys.modules, "src.config", mod)
    return pkg.Renderer(pkg.Network())


def test_train_task_constructs_and_perturbs(monkeypatch):
    ren = _renderer_with_cfg(monkeypatch, task="train")
    assert ren.task == "train" and ren.perturb is True
    ren = _renderer_with_cfg(monkeypatch, task="train", perturb=0)
    assert ren.perturb is False
    ren = _renderer_with_cfg(monkeypatch, task="test", perturb=1)
    assert ren.perturb is False                        # the reference turns perturb off outside training


def test_draws_follow_the_reference_order(monkeypatch):
    ren = _renderer_with_cfg(monkeypatch, task="train")
    calls = []

    def rand(shape, device):
        calls.append(tuple(shape))
        return torch.full(shape, 0.5)
    ren._rand = rand
    jitter, u = ren._draws(8, torch.device("cpu"))
    assert calls == [(8, 64), (8, 128)] and jitter.shape == (8, 64) and u.shape == (8, 128)
    calls.clear()
    ren.perturb = False                                # read at call time, as the reference does
    jitter, u = ren._draws(8, torch.device("cpu"))
    assert calls == [(8, 128)] and jitter is None
    calls.clear()
    ren.task, ren.perturb = "test", True
    jitter, u = ren._draws(8, torch.device("cpu"))
    assert calls == [(8, 64)] and u is None
    # torch.manual_seed controls the default draw
    ren = _renderer_with_cfg(monkeypatch, task="train")
    torch.manual_seed(3)
    a = ren._draws(4, torch.device("cpu"))
    torch.manual_seed(3)
    b = ren._draws(4, torch.device("cpu"))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_restatement_reproduces_reference_bit_for_bit(oracle, golden, synthetic_sd):
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    g = golden("stochastic_render.npz")
    o, d = g["rays_o"], g["rays_d"]
    for tag, fam, jitter, u in SC.fixture_runs(g):
        sd = SC.family_sd(oracle, synthetic_sd, fam)
        with torch.no_grad():
            rgb, dep, parts = SC.render(sd, o, d, jitter, u)
        assert torch.equal(parts["raw_coarse"][..., 3], g[f"{tag}_sigma_coarse_raw"]), tag
        assert torch.equal(parts["t_sorted"], g[f"{tag}_t_sorted"]), tag
        assert torch.equal(rgb, g[f"{tag}_rgb"]) and torch.equal(dep, g[f"{tag}_depth"]), tag


def test_stratified_restatement_is_the_elementwise_expression():
    j = torch.tensor([[0.0] * 64, [torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)).item()] * 64])
    t = SC.stratified_t(j)
    lin = torch.linspace(2.0, 6.0, 64)
    assert t[0, 0] == lin[0] and t[1, -1] <= lin[-1] and torch.all(t[:, 1:] >= t[:, :-1])


def test_new_symbols_in_header_binding_and_library():
    import re
    import nerf_replication_amd._lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "nerf_mi355x.h")).read(), flags=re.S)
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in L._PROTOS, name
        assert hasattr(lib, name), name
    lib.nerf_abi_version.restype = ctypes.c_int32
    assert lib.nerf_abi_version() == 3
    ws = lib.nerf_render_stochastic_workspace_bytes
    ws.restype, ws.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]
    det = lib.nerf_render_workspace_bytes
    det.restype, det.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    # the deterministic workspace + the jittered depths [n,64] of one ray block
    assert ws(640000, 128) == det(640000, 128, 0) + 640000 * 256
    assert ws(10 ** 8, 0) == det(1 << 20, 0, 0) + (1 << 20) * 256
    assert ws(-1, 128) == -1

