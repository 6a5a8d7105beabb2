"""CPU checks of the hash-grid radiance field: the restatement (tests/hashfield_reference.py) against itself -- the SH basis is
orthonormal, its fp32 fixed-order form is accurate, the hand-composed float64 backward is torch autograd's -- and the host surface:
header against binding table, exported names, lazy import, state-dict keys, and every refusal that happens before the library (or
before any launch) is reached."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hashfield_reference as R
from conftest import REPO
from test_fused_mlp_cpu import NN_HEADER, _declared_signatures

NEW_ENTRIES = ("nerf_sh4_encode", "nerf_field_points", "nerf_field_color_inputs", "nerf_field_color_inputs_backward",
               "nerf_field_raw_scatter", "nerf_field_raw_gather")


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_sh_basis_is_orthonormal():
    """Gauss-Legendre with 8 nodes in z and 16 uniform nodes in phi integrates products of two degree-3 harmonics exactly."""
    gram = R.sh_gram(8, 16)
    dev = float((gram - torch.eye(16, dtype=torch.float64)).abs().max())
    print("max deviation from the identity", dev)
    assert dev <= 1e-12


def sh_test_directions():
    gen = torch.Generator().manual_seed(11)
    d = torch.randn(1000, 3, generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    for i, axis in enumerate(torch.eye(3)):
        d[2 * i], d[2 * i + 1] = axis, -axis
    d[6] = d[6] * 1e-3                               # a direction of length 1e-3 before normalisation
    return d


def test_sh_fp32_form_is_within_4_ulp():
    """fp32, fixed order (normalisation included) against float64 on 1000 directions, +-axes and a short one among them: every
    coefficient within 4 ulp, one ulp being 2^-23, the fp32 ulp of 1.0 (hashfield_reference.SH_ULP)."""
    d = sh_test_directions()
    f32, f64 = R.sh4(d, torch.float32), R.sh4(d, torch.float64)
    assert f32.dtype == torch.float32 and f64.dtype == torch.float64
    err = ((f32.double() - f64).abs() / R.SH_ULP).max(dim=0).values
    print("max error per coefficient, ulp:", [round(float(e), 3) for e in err])
    assert bool((err <= 4.0).all())
    # the +-axes are exact where the formula is a product with an exact zero
    assert f32[4, 1] == 0 and f32[4, 3] == 0 and float(f32[4, 2]) == float(np.float32(0.48860251190291987))


def test_glue_restatements_are_inverse_and_fp32():
    gen = torch.Generator().manual_seed(3)
    n, S = 7, 5
    o, d = R.make_rays(n, 1)
    t = torch.linspace(2.0, 6.0, S)
    frame = R.box_frame(R.BBOX)
    assert frame[2] == float(np.float32(3.0 + 1e-6))
    index = torch.tensor([0, 3, 4, 9, 21, 34], dtype=torch.int32)
    x = R.points(o, d, t, S, index, 6, frame)
    assert x.dtype == torch.float32 and float(x.min()) >= 0 and float(x.max()) <= 1
    # ray 1 starts at (9, 9, 9) and looks along +x: every sample is clamped to the box's corner
    x_all = R.points(o, d, t, S, None, n * S, frame)
    assert torch.equal(x_all[S:2 * S], torch.full((S, 3), float(np.float32(3.0) / np.float32(frame[2]))))
    assert torch.equal(x, x_all[index.long()])
    # point mode is the same normalisation of the points themselves
    p = o[index.long() // S] + d[index.long() // S] * t[index.long() % S][:, None]
    assert torch.equal(R.points(p, None, None, 1, None, 6, frame), x)
    geo, sh = torch.randn(6, 16, generator=gen), R.sh4(d)
    cin, sig = R.color_inputs(geo, sh, S, index, 6)
    assert torch.equal(cin[:, :16], geo) and torch.equal(cin[:, 16:], sh[index.long() // S]) and torch.equal(sig, geo[:, 0])
    rgb = torch.randn(6, 3, generator=gen)
    raw = R.raw_scatter(rgb, sig, index, 6, n * S)
    assert float(raw.abs().sum(1).ne(0).sum()) == 6
    back = R.raw_gather(raw, index, 6)
    assert torch.equal(back[0], rgb) and torch.equal(back[1], sig)
    g = R.color_inputs_backward(cin, sig)
    assert torch.equal(g[:, 1:], geo[:, 1:]) and torch.equal(g[:, 0], geo[:, 0] + sig)


def test_fp32_hash_forward_is_hashgrid_references():
    import hashgrid_reference as H
    sc = R.scene(5, 3)
    x = R.points(sc["o"], sc["d"], sc["t"], 3, None, 15, sc["frame"])
    assert torch.equal(R.hash_forward(x, sc["params"]["emb"], sc["offsets"], sc["scales"]),
                       H.forward_f32(x, sc["params"]["emb"], sc["offsets"], sc["scales"]))


@pytest.mark.parametrize("white", [1, 0])
@pytest.mark.parametrize("culled", [False, True])
def test_composed_backward_is_autograd(white, culled):
    """The float64 gradients composed by hand from the pieces (render_backward) against torch autograd through render(), for every
    parameter tensor, to 1e-10."""
    n, S = 9, 5
    sc = R.scene(n, S)
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    b = torch.randn(n, generator=gen, dtype=torch.float64)
    keep = (torch.rand(n, S, generator=gen) > 0.4) if culled else None
    args = (sc["o"], sc["d"], sc["t"], sc["frame"], white, sc["offsets"], sc["scales"])
    p64 = R.cast_params(sc["params"], torch.float64, requires_grad=True)
    (rgb, depth), pres = R.render(p64, *args, keep=keep, want_pres=True)
    assert 0.2 < float((pres[-1] > 0).double().mean()) < 0.8            # the scene is neither empty nor solid
    ((rgb * a).sum() + (depth * b).sum()).backward()
    by_hand = R.render_backward(sc["params"], *args, a, b, keep=keep)
    worst = max(float((p.grad - g).abs().max()) for p, g in zip(R.flat_params(p64), by_hand))
    print("max |by hand - autograd|", worst)
    assert worst <= 1e-10
    assert all(float(p.grad.abs().max()) > 0 for p in R.flat_params(p64))


def test_fp32_restatement_follows_the_float64_one():
    sc = R.scene(9, 5)
    args = (sc["o"], sc["d"], sc["t"], sc["frame"], 1, sc["offsets"], sc["scales"])
    r32, d32 = R.render(R.cast_params(sc["params"], torch.float32), *args)
    r64, d64 = R.render(R.cast_params(sc["params"], torch.float64), *args)
    assert r32.dtype == torch.float32 and float((r32.double() - r64).abs().max()) < 1e-5
    assert float((d32.double() - d64).abs().max()) < 1e-4
    assert torch.isfinite(r64).all() and torch.isfinite(d64).all()


# ---- the host surface ------------------------------------------------------------------------------------------------------------------
def test_header_and_table_agree_on_the_new_entries():
    import nerf_replication_amd._lib as L
    declared = _declared_signatures(NN_HEADER)
    for name in NEW_ENTRIES:
        assert name in L.NN_EXPORTS and L.NN_SIGNATURES[name] == declared[name], name
        assert L.NN_SIGNATURES[name][0] == "status"
    assert sorted(declared) == sorted(L.NN_EXPORTS) and len(L.NN_EXPORTS) == 11
    assert len(L.EXPORTS) == 65                                   # the core table does not move
    assert L.NN_SIGNATURES["nerf_field_points"][1][8:10] == ("f32[3]", "f32[3]")


def test_library_exports_the_new_entries():
    import nerf_replication_amd._lib as L
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert L.load().nerf_nn_abi_version() == 1 and L.load().nerf_abi_version() == 3


def test_entries_refuse_before_any_launch():
    """Sizes and pointers outside the contract come back as NERF_ERR_INVALID_ARG with a message; the refusal is host code, so this
    runs without a GPU (the pointers are never followed)."""
    import nerf_replication_amd._lib as L
    lib = L.load()
    p, odd = 0x10000, 0x10004
    box = (ctypes.c_float * 3)(0, 0, 0)
    INVALID = -1

    def refused(rc):
        assert rc != 0 and lib.nerf_last_error()
        return rc
    assert lib.nerf_abi_version() == 3
    bad = [
        lib.nerf_sh4_encode(p, 0, p, None), lib.nerf_sh4_encode(None, 4, p, None), lib.nerf_sh4_encode(p, 4, odd, None),
        lib.nerf_sh4_encode(p, 2 ** 31, p, None),
        lib.nerf_field_points(p, p, p, 0, 4, 3, None, 0, box, box, 1.0, p, None),               # n_rows <= 0
        lib.nerf_field_points(p, p, p, 0, 4, 3, None, 13, box, box, 1.0, p, None),              # more rows than points
        lib.nerf_field_points(p, p, p, 0, 4, 0, None, 1, box, box, 1.0, p, None),               # n_samples outside [1, 192]
        lib.nerf_field_points(p, p, p, 0, 4, 193, None, 1, box, box, 1.0, p, None),
        lib.nerf_field_points(p, p, p, 0, 2 ** 31 // 192 + 1, 192, None, 1, box, box, 1.0, p, None),      # n_rays * n_samples > 2^31 - 1
        lib.nerf_field_points(None, p, p, 0, 4, 3, None, 1, box, box, 1.0, p, None),
        lib.nerf_field_points(p, p, None, 0, 4, 3, None, 1, box, box, 1.0, p, None),            # rays without depths
        lib.nerf_field_points(p, None, None, 0, 4, 3, None, 1, box, box, 1.0, p, None),         # point mode needs n_samples == 1
        lib.nerf_field_points(p, p, p, 0, 4, 3, None, 1, box, box, 0.0, p, None),               # extent
        lib.nerf_field_points(p, p, p, 0, 4, 3, None, 1, None, box, 1.0, p, None),
        lib.nerf_field_color_inputs(p, p, None, 0, 4, 3, p, p, None), lib.nerf_field_color_inputs(p, p, None, 5, 4, 193, p, p, None),
        lib.nerf_field_color_inputs(p, None, None, 5, 4, 3, p, p, None), lib.nerf_field_color_inputs(p, p, None, 5, 4, 3, odd, p, None),
        lib.nerf_field_color_inputs(p, p, None, 5, 4, 3, p, None, None),
        lib.nerf_field_color_inputs_backward(p, p, 0, p, None), lib.nerf_field_color_inputs_backward(p, None, 5, p, None),
        lib.nerf_field_color_inputs_backward(odd, p, 5, p, None), lib.nerf_field_color_inputs_backward(p, p, 2 ** 31, p, None),
        lib.nerf_field_raw_scatter(p, p, None, 0, 12, p, None), lib.nerf_field_raw_scatter(p, p, None, 13, 12, p, None),
        lib.nerf_field_raw_scatter(p, p, None, 5, 2 ** 31, p, None), lib.nerf_field_raw_scatter(p, None, None, 5, 12, p, None),
        lib.nerf_field_raw_scatter(p, p, None, 5, 12, odd, None),
        lib.nerf_field_raw_gather(p, None, 0, 12, p, p, None), lib.nerf_field_raw_gather(p, None, 13, 12, p, p, None),
        lib.nerf_field_raw_gather(None, None, 5, 12, p, p, None), lib.nerf_field_raw_gather(odd, None, 5, 12, p, p, None),
    ]
    assert [refused(rc) for rc in bad] == [INVALID] * len(bad)


def test_public_names_are_lazy():
    import nerf_replication_amd as pkg
    for name in ("HashField", "HashRenderer"):
        assert name in pkg.__all__ and name in dir(pkg) and callable(getattr(pkg, name)), name
    assert "hashfield" in pkg._SUBMODULES
    code = ("import sys; sys.path.insert(0, %r); import nerf_replication_amd as p; "
            "assert not [m for m in sys.modules if m.startswith('nerf_replication_amd.')], sys.modules.keys(); "
            "assert p.HashRenderer.__module__ == 'nerf_replication_amd.hashfield'" % REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def small_field(pkg, L=4, T=12, **kwargs):
    enc = pkg.HashEncoder(input_dim=3, num_levels=L, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=T)
    return pkg.HashField(R.BBOX, encoder=enc, **kwargs)


def test_state_dict_and_structure():
    import nerf_replication_amd as pkg
    field = small_field(pkg)
    keys = ["encoder.embeddings"] + [f"sigma_net.layers.{i}.{p}" for i in range(2) for p in ("weight", "bias")] + \
           [f"color_net.layers.{i}.{p}" for i in range(3) for p in ("weight", "bias")] + ["wbounds"]
    sd = field.state_dict()
    assert sorted(sd.keys()) == sorted(keys)
    assert len(list(field.parameters())) == 11 and [n for n, _ in field.named_buffers()] == ["wbounds"]
    assert sd["wbounds"].dtype == torch.float32 and sd["wbounds"].tolist() == list(R.BBOX)
    assert list(sd["sigma_net.layers.0.weight"].shape) == [64, 8] and list(sd["sigma_net.layers.1.weight"].shape) == [16, 64]
    assert list(sd["color_net.layers.0.weight"].shape) == [64, 32] and list(sd["color_net.layers.2.weight"].shape) == [3, 64]
    assert field.encoder.out_dim == 8 and isinstance(field.sigma_net, pkg.FusedMLP)
    # the density starts positive (a uniform fog): relu(sigma) of a field that starts negative everywhere has no gradient at all
    assert float(field.sigma_net.layers[-1].bias.detach()[0]) == 1.0
    # the default encoder: 16 levels of 2 channels, 2^19 rows at most, resolution 16 .. 2048
    default = pkg.HashField(R.BBOX)
    enc = default.encoder
    assert (enc.num_levels, enc.level_dim, enc.base_resolution, enc.log2_hashmap_size, enc.out_dim) == (16, 2, 16, 19, 32)
    assert abs(16 * enc.per_level_scale ** 15 - 2048) < 1e-6 and len(list(default.parameters())) == 11
    assert list(default.sigma_net.layers[0].weight.shape) == [64, 32]
    # a checkpoint carries the box, and the host frame follows a load
    other = pkg.HashField((-1, -2, -3, 1, 2, 5), encoder=pkg.HashEncoder(input_dim=3, num_levels=4, log2_hashmap_size=12))
    assert other.frame()[2] == float(np.float32(8.0 + 1e-6)) and other.bbox.tolist() == [-1, -2, -3, 1, 2, 5]
    other.load_state_dict(sd)
    lo, hi, extent = other.frame()
    assert lo == (-1.5,) * 3 and hi == (1.5,) * 3 and extent == R.box_frame(R.BBOX)[2]
    renderer = pkg.HashRenderer(field)
    assert renderer.net is field and renderer.field is field
    assert (renderer.N_samples, renderer.t_near, renderer.t_far, renderer.white_bkgd, renderer.occupancy, renderer.chunk_rays,
            renderer.stats) == (192, 2.0, 6.0, True, None, 16384, None)
    for bad in (dict(geo_dim=8), dict(width=96), dict(sigma_hidden=0)):
        with pytest.raises(ValueError):
            small_field(pkg, **bad)
    with pytest.raises(ValueError):
        pkg.HashField((0, 0, 0, 1, 1, 0))
    with pytest.raises(TypeError):
        pkg.HashField(R.BBOX, encoder=pkg.HashEncoder(input_dim=2, num_levels=2, log2_hashmap_size=8))
    with pytest.raises(TypeError):
        pkg.HashRenderer(torch.nn.Linear(2, 2))


def test_refusals_before_the_library(monkeypatch):
    import nerf_replication_amd as pkg
    from nerf_replication_amd import _lib

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", reached)
    field = small_field(pkg)
    renderer = pkg.HashRenderer(field)
    rays = {"rays_o": torch.zeros(1, 4, 3), "rays_d": torch.ones(1, 4, 3)}
    with pytest.raises(_lib.NerfLibraryError):                     # CPU rays: no fallback
        renderer.render(rays)
    with pytest.raises(_lib.NerfLibraryError):
        field.density(torch.zeros(5, 3))
    with pytest.raises(NotImplementedError):                       # no ray adjoint
        renderer.render({"rays_o": torch.zeros(1, 4, 3, requires_grad=True), "rays_d": torch.ones(1, 4, 3)})
    with pytest.raises(NotImplementedError):
        renderer.render({"rays_o": torch.zeros(1, 4, 3), "rays_d": torch.ones(1, 4, 3, requires_grad=True)})
    for bad in (0, 193, -1, 64.0, True, None):
        renderer.N_samples = bad
        with pytest.raises(ValueError):
            renderer.render(rays)
    renderer.N_samples = 64
    renderer.occupancy = object()
    with pytest.raises(TypeError, match="must be an OccupancyGrid or None"):
        renderer.render(rays)
    renderer.occupancy = None
    renderer.chunk_rays = 0
    with pytest.raises(ValueError):
        renderer.render(rays)
    renderer.chunk_rays = 16384
    with pytest.raises(ValueError):
        renderer.render({"rays_o": torch.zeros(4, 3), "rays_d": torch.ones(4, 3)})
    half = pkg.HashRenderer(small_field(pkg).half())
    with pytest.raises(NotImplementedError):                       # fp32 parameters only
        half.render(rays)
    with pytest.raises(NotImplementedError):
        field.density(torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        field.density(torch.zeros(5, 2))
