"""CPU checks of the hash field's sampling: the fp32 restatement of nerf_field_sample_importance
(tests/hashfield_sampling_reference.py) against a float64 version of the reference's expressions, the stratified restatement against
the torch expression, include/nerf_mi355x_sampling.h against its binding table, the host refusals of the new entries through the C
ABI, and HashRenderer's refusals that happen before the library is reached."""
import ctypes
import os

import pytest
import torch

import hashfield_reference as R
import hashfield_sampling_reference as SR
from conftest import REPO
from test_fused_mlp_cpu import _declared_signatures, _declared_symbols

HEADER = os.path.join(REPO, "include", "nerf_mi355x_sampling.h")
NEW_ENTRIES = ("nerf_field_sample_importance", "nerf_field_stratified_depths", "nerf_field_density_scatter")
COUNTS = [(3, 1), (3, 189), (4, 5), (33, 64), (64, 128), (190, 2)]


def rays_of_weights(n, Sc, seed):
    """n >= 6 rays of weights [n,Sc]: all zero, one-hot at the first interior sample, one-hot at the last interior sample, nonzero
    only at samples 0 and Sc - 1 (both ignored), 1e-30 everywhere, then random ones (a few peaks over a floor of zeros)."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.rand(n, Sc, generator=gen) * (torch.rand(n, Sc, generator=gen) < 0.3)
    w[0] = 0.0
    w[1] = 0.0
    w[1, 1] = 1.0
    w[2] = 0.0
    w[2, Sc - 2] = 1.0
    w[3] = 0.0
    w[3, 0], w[3, Sc - 1] = 0.7, 0.3
    w[4] = 1e-30
    return w.contiguous()


def us_of(n, Sf, seed):
    """u [n,Sf] in [0, 1], unsorted, every ray holding 0, 1 and 1 - 2^-24 (Sf < 3: as many of them as fit, another choice per ray)."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(n, Sf, generator=gen)
    special = [0.0, 1.0, 1.0 - 2.0 ** -24]
    for r in range(n):
        for k in range(min(3, Sf)):
            u[r, (r + 7 * k) % Sf] = special[k if Sf >= 3 else (k + r) % 3]
    return u.contiguous()


def depths_of(n, Sc, seed):
    """Ascending depths per ray in [2, 6]: the stratified jitter of the linspace table."""
    gen = torch.Generator().manual_seed(seed)
    return SR.stratified(torch.linspace(2.0, 6.0, Sc), torch.rand(n, Sc, generator=gen)).contiguous()


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sc,Sf", COUNTS)
@pytest.mark.parametrize("per_ray", [False, True])
def test_restatement_properties(Sc, Sf, per_ray):
    n, K = 9, Sc - 2
    w = rays_of_weights(n, Sc, Sc * 1000 + Sf)
    t = depths_of(n, Sc, 5) if per_ray else torch.linspace(2.0, 6.0, Sc)
    u = us_of(n, Sf, 6) if per_ray else torch.sort(us_of(1, Sf, 6)[0]).values
    merged, fine = SR.sample_importance(w, t, u)
    tt = SR._rows(t, n)
    bins = 0.5 * (tt[:, 1:] + tt[:, :-1])
    assert merged.shape == (n, Sc + Sf) and fine.shape == (n, Sf) and merged.dtype == torch.float32
    assert bool((merged[:, 1:] >= merged[:, :-1]).all())                          # ascending
    for r in range(n):                                                            # the union, as multisets
        assert torch.equal(merged[r], torch.sort(torch.cat([tt[r], fine[r]])).values)
    assert bool((fine >= bins[:, :1]).all()) and bool((fine <= bins[:, K:K + 1]).all())
    # u >= cdf_K gives the last edge exactly (cdf_K is 1 up to rounding: u = 1 is not always there), u = 0 the first
    uu = SR._rows(u, n)
    top = uu >= SR.cdf_of(w)[:, K:K + 1]
    assert (Sf < 3 or int(top.sum()) > 0) and torch.equal(fine[top], bins[:, K:K + 1].expand(n, Sf)[top])
    assert torch.equal(fine[uu == 0.0], bins[:, :1].expand(n, Sf)[uu == 0.0])
    # rays 0 (all zero), 3 (only the two ignored samples) and 4 (1e-30 everywhere) have the same interior weights after + 1e-5
    t0, u0 = tt[0:1].contiguous(), uu[0:1].contiguous()
    assert torch.equal(fine[0], SR.sample_importance(w[3:4], t0, u0)[1][0])
    assert torch.equal(fine[0], SR.sample_importance(w[4:5], t0, u0)[1][0])


@pytest.mark.parametrize("Sc,Sf", [(4, 5), (33, 64), (64, 128)])
def test_restatement_against_float64(Sc, Sf):
    """Where both arithmetics put a u between the same two cdf entries and the interval is not degenerate, the fp32 depth is the
    float64 one up to the conditioning of the interpolation: errors of at most (K + 8) u_32 in cdf and u - cdf (K sequential sums of
    values <= 1) move frac by that over denom, and the depth by that times the bin width, plus a few ulps of the depth itself."""
    n, K = 12, Sc - 2
    w = rays_of_weights(n, Sc, 3)
    t, u = depths_of(n, Sc, 8), us_of(n, Sf, 9)
    _, fine = SR.sample_importance(w, t, u)
    merged64, fine64, aux = SR.sample_importance_f64(w, t, u)
    assert bool((merged64[:, 1:] >= merged64[:, :-1]).all())
    below = torch.clamp(aux["inds"] - 1, 0, K)
    above = torch.clamp(aux["inds"], 0, K)
    width = torch.gather(aux["bins"], 1, above) - torch.gather(aux["bins"], 1, below)
    tol = width * (K + 8) * 2.0 ** -23 / aux["denom"] + 8 * 2.0 ** -21
    err = (fine.double() - fine64).abs()
    ok = err <= tol
    # a u within rounding of a cdf entry may fall to the other side in fp32: a different, adjacent interval (few)
    print("outside the tolerance:", int((~ok).sum()), "of", ok.numel(), "largest error / tolerance", float((err / tol).max()))
    assert float((~ok).double().mean()) <= 0.02
    assert float(err.max()) <= float(width.max()) + 1e-5


def test_all_zero_ray_spreads_uniformly():
    """Equal interior weights: cdf_i = i / K up to rounding, so u = (k + 0.5) / Sf lands at the same fraction of [bins_0, bins_K]
    when the coarse depths are equidistant."""
    Sc, Sf = 34, 64
    K = Sc - 2
    t = torch.linspace(2.0, 6.0, Sc)
    u = (torch.arange(Sf, dtype=torch.float32) + 0.5) / Sf
    _, fine = SR.sample_importance(torch.zeros(1, Sc), t, u)
    bins = 0.5 * (t[1:] + t[:-1])
    want = bins[0].double() + u.double() * (bins[K] - bins[0]).double()
    assert float((fine[0].double() - want).abs().max()) <= 64 * 2.0 ** -23 * 6.0
    gaps = fine[0, 1:] - fine[0, :-1]
    assert float(gaps.min()) > 0 and float(gaps.max() / gaps.min()) < 1.001


@pytest.mark.parametrize("Sc,hot", [(3, 1), (4, 1), (4, 2), (33, 1), (33, 17), (33, 31), (190, 188)])
def test_one_hot_weight_fills_its_two_bins(Sc, hot):
    """All of the mass at interior sample `hot`: pdf entry hot - 1, the interval [bins_{hot-1}, bins_hot] -- every fine depth whose u is
    not within the 1e-5 floor's share of the ends lies there."""
    K, Sf = Sc - 2, 50
    w = torch.zeros(1, Sc)
    w[0, hot] = 1.0
    t = torch.linspace(2.0, 6.0, Sc)
    u = torch.linspace(0.01, 0.99, Sf)                                            # the floor holds (K - 1) * 1e-5 < 0.002 of the mass
    _, fine = SR.sample_importance(w, t, u)
    bins = 0.5 * (t[1:] + t[:-1])
    assert bool((fine >= bins[hot - 1]).all()) and bool((fine <= bins[hot]).all())
    assert K >= 1


@pytest.mark.parametrize("S", [1, 2, 3, 64, 192])
def test_stratified_restatement(S):
    t = torch.linspace(2.0, 6.0, S)
    gen = torch.Generator().manual_seed(S)
    jit = torch.rand(7, S, generator=gen)
    jit[0], jit[1] = 0.0, 1.0 - 2.0 ** -24
    got = SR.stratified(t, jit)
    # element by element, every operation on its own (the kernel's form)
    want = torch.empty_like(got)
    for s in range(S):
        lower = t[0] if s == 0 else 0.5 * (t[s] + t[s - 1])
        upper = t[S - 1] if s == S - 1 else 0.5 * (t[s + 1] + t[s])
        want[:, s] = lower + (upper - lower) * jit[:, s]
    assert torch.equal(got, want) and got.dtype == torch.float32
    assert bool((got[:, 1:] >= got[:, :-1]).all())
    lower0 = torch.cat([t[:1], 0.5 * (t[1:] + t[:-1])])
    assert torch.equal(got[0], lower0)                                            # jitter 0: the lower edges, S == 1: t0
    if S == 1:
        assert torch.equal(got, t.expand(7, 1))


# ---- the host surface ------------------------------------------------------------------------------------------------------------------
def test_sampling_header_declares_its_table():
    import nerf_replication_amd._lib as L
    declared = _declared_signatures(HEADER)
    assert sorted(declared) == _declared_symbols(HEADER) == sorted(L.SAMPLING_EXPORTS) == sorted(NEW_ENTRIES)
    assert tuple(L._SAMPLING_PROTOS) == L.SAMPLING_EXPORTS == tuple(L.SAMPLING_SIGNATURES)
    for name in NEW_ENTRIES:
        assert L.SAMPLING_SIGNATURES[name] == declared[name] and L.SAMPLING_SIGNATURES[name][0] == "status", name
        assert len(L._SAMPLING_PROTOS[name][1]) == len(declared[name][1])
    earlier = (L.EXPORTS, L.NN_EXPORTS, L.FIELD_EXPORTS, L.HASHGRID_EXPORTS, L.NN_EXACT_EXPORTS, L.ORDER_EXPORTS)
    assert not set(L.SAMPLING_EXPORTS) & set().union(*map(set, earlier))
    assert tuple(len(e) for e in earlier) == (65, 11, 4, 3, 3, 3)                 # the earlier tables do not move


def test_library_exports_the_sampling_entries():
    import nerf_replication_amd._lib as L
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert L.load().nerf_nn_abi_version() == 1 and L.load().nerf_abi_version() == 3


def test_entries_refuse_before_any_launch():
    """Host code: the pointers are never followed, so this runs without a GPU."""
    import nerf_replication_amd._lib as L
    lib = L.load()
    p, odd, odd16 = 0x10000, 0x10002, 0x10004

    def si(w=p, t=p, ts=0, u=p, us=0, n=4, Sc=8, Sf=8, merged=p, fine=None):
        return lib.nerf_field_sample_importance(w, t, ts, u, us, n, Sc, Sf, merged, fine, None)

    def sd(tab=p, jit=p, n=4, S=8, out=p):
        return lib.nerf_field_stratified_depths(tab, jit, n, S, out, None)

    def ds(sigma=p, stride=16, index=None, rows=5, points=12, raw=p):
        return lib.nerf_field_density_scatter(sigma, stride, index, rows, points, raw, None)
    bad = [
        si(w=None), si(t=None), si(u=None), si(merged=None), si(w=odd), si(t=odd), si(u=odd), si(merged=odd), si(fine=odd),
        si(Sc=2), si(Sf=0), si(Sc=-1), si(Sc=100, Sf=93), si(Sc=192, Sf=1), si(n=0), si(n=-1), si(n=2 ** 31 // 16 + 1),
        si(ts=1), si(ts=16), si(ts=-8), si(us=1), si(us=16), si(us=-8), si(Sc=8, Sf=4, us=8),
        sd(tab=None), sd(jit=None), sd(out=None), sd(tab=odd), sd(jit=odd), sd(out=odd), sd(S=0), sd(S=193), sd(n=0),
        sd(n=2 ** 31 // 8 + 1),
        ds(sigma=None), ds(raw=None), ds(sigma=odd), ds(index=odd), ds(raw=odd16), ds(stride=0), ds(rows=0), ds(rows=13), ds(points=0),
        ds(rows=5, points=2 ** 31),
    ]
    for i, rc in enumerate(bad):
        assert rc == -1 and lib.nerf_last_error(), i


def small_field(pkg):
    enc = pkg.HashEncoder(input_dim=3, num_levels=4, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=12)
    return pkg.HashField(R.BBOX, encoder=enc)


def test_refusals_before_the_library(monkeypatch):
    import nerf_replication_amd as pkg
    from nerf_replication_amd import _lib

    def reached(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "call", reached)
    ren = pkg.HashRenderer(small_field(pkg))
    assert ren.N_importance == 0 and ren.perturb is False and ren.samples is None and ren.N_samples == 192
    monkeypatch.setattr(ren, "_rand", reached)
    rays = {"rays_o": torch.zeros(1, 4, 3), "rays_d": torch.ones(1, 4, 3)}
    grad_rays = {"rays_o": torch.zeros(1, 4, 3, requires_grad=True), "rays_d": torch.ones(1, 4, 3)}
    ren.N_samples = 64
    for bad in (-1, 129, 1.0, True, None, "8"):                   # an int in [0, 192 - N_samples]
        ren.N_importance = bad
        for call in (ren.render, ren.render_geometry):
            with pytest.raises(ValueError, match="N_importance"):
                call(rays)
    for Sc in (1, 2):                                             # resampling needs an interior weight
        ren.N_samples, ren.N_importance = Sc, 8
        for call in (ren.render, ren.render_geometry):
            with pytest.raises(ValueError, match="N_samples >= 3"):
                call(rays)
    ren.N_samples, ren.N_importance = 64, 128
    for bad in (0, 1, None, "yes", 1.0):
        ren.perturb = bad
        for call in (ren.render, ren.render_geometry):
            with pytest.raises(ValueError, match="perturb"):
                call(rays)
    ren.perturb = True
    with pytest.raises(NotImplementedError, match="perturb"):
        ren.render_geometry(rays)
    ren.perturb = False
    ren.ray_gradients = True
    with pytest.raises(NotImplementedError, match="N_importance"):
        ren.render(grad_rays)
    ren.N_importance = 0
    with pytest.raises(_lib.NerfLibraryError):                    # without resampling the ray adjoint goes as far as it did: to a GPU
        ren.render(grad_rays)
    ren.ray_gradients = False
    ren.N_importance = 128
    with pytest.raises(_lib.NerfLibraryError):                    # a valid setting on CPU rays: no fallback
        ren.render(rays)
    with pytest.raises(_lib.NerfLibraryError):
        ren.render_geometry(rays)
