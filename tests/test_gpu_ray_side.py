"""GPU tests of the NeRF path's ray side on edge rays (tests/ray_side_reference.py): nerf_sample_fine / nerf_sample_fine_rays (with the
ESS/ERT masks) and nerf_composite (staged and simple kernel) bit for bit on every ray, and the two adjoints under the project's rule

    max|hip - f64| <= 3 * max|cpu_fp32 - f64| + 2 u max|f64|,   u = 2^-24,

per family of rays and per output tensor, every ray divided by its own max|f64| (a ray whose float64 gradient is zero is exactly zero
on the device), with f64 and cpu_fp32 the two evaluations of the restatement's twin on the decisions of the fp32 restatement.

The forward kernels are IEEE arithmetic except for expf.  The device's own expf enters the restatement through probes of the public
ABI: alpha(sigma, delta) is weights[0] of nerf_composite on the two-sample ray raw = [(0, 0, 0, sigma), 0], t = (0, delta) (T = 1, so
w = alpha, and fsub(delta, 0) = delta exactly), the last sample's alpha (delta = 1e10) is weights[0] of a one-sample ray, and
sigmoid(x) is the rgb of a one-sample opaque ray without background (w = 1 exactly).  The probes are held to float64 themselves.
Measured / allowed go to profiles/ray_side.json.

Measured on the MI355X: probes 0.97 u (alpha) and 1.46 u (sigmoid); every forward comparison bit-equal; the adjoints at most 5.8e-8 of
a ray's largest gradient from float64 in every family.  (With their smooth part in fp32 the two adjoint kernels missed the rule in 22
compositing cases and one sampler family, by factors up to 2.6: behind a nearly opaque sample fp32's 1 - alpha sits on a grid of
2^-24, and the device's expf and the CPU's exp fall on different sides of it.  They now evaluate everything but the decisions in
float64.)"""
import pytest
import torch

import ray_side_reference as RS
from gpu_common import amd  # noqa: F401
from test_gpu_hashfield import Guarded, same
from test_ray_side_reference_cpu import STRIDES          # (t stride, u table) of RS.sampler_tables

pytestmark = pytest.mark.gpu

U = RS.U
NAN = float("nan")
BYTE_SENTINEL = 0xA5


class GuardedBytes:
    """test_gpu_hashfield.Guarded for a uint8 output (its float sentinel does not fit a byte)."""

    def __init__(self, shape):
        n = int(torch.tensor(shape).prod())
        self.whole = torch.full((n + 512,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
        self.view = self.whole[256:256 + n].view(shape)

    def intact(self):
        w = self.whole.cpu()
        return bool((w[:256] == BYTE_SENTINEL).all() and (w[-256:] == BYTE_SENTINEL).all())


# ---- device probes ---------------------------------------------------------------------------------------------------------------------
def device_alpha(amd):
    """-> alpha_of(sigma, delta) for float32 CPU tensors, read from the device."""
    def alpha_of(sigma, delta):
        s, d = sigma.reshape(-1).contiguous(), delta.expand_as(sigma).reshape(-1).contiguous()
        out = torch.empty_like(s)
        last = d == torch.tensor(1e10, dtype=torch.float32)
        for sel, S in ((~last, 2), (last, 1)):
            m = int(sel.sum())
            if m == 0:
                continue
            raw, t = torch.zeros(m, S, 4), torch.zeros(m, S)
            raw[:, 0, 3] = s[sel]
            if S == 2:
                t[:, 1] = d[sel]
            rgb, dep, w = (torch.empty(m, 3, device="cuda"), torch.empty(m, device="cuda"), torch.empty(m, S, device="cuda"))
            amd._lib.call("nerf_composite", raw.cuda(), t.cuda(), S, m, S, 0, rgb, dep, w)
            out[sel] = w[:, 0].cpu()
        return out.view(sigma.shape)
    return alpha_of


def device_sigmoid(amd):
    def sigmoid(x):
        flat = x.reshape(-1)
        m = (flat.numel() + 2) // 3
        raw = torch.zeros(m, 1, 4)
        cols = torch.zeros(m * 3)
        cols[:flat.numel()] = flat
        raw[:, 0, :3] = cols.view(m, 3)
        raw[:, 0, 3] = RS.OPAQUE                                     # times 1e10: exp underflows to 0, alpha = 1, w = 1
        rgb, dep = torch.empty(m, 3, device="cuda"), torch.empty(m, device="cuda")
        amd._lib.call("nerf_composite", raw.cuda(), torch.full((m, 1), 2.0).cuda(), 1, m, 1, 0, rgb, dep, None)
        return rgb.cpu().reshape(-1)[:flat.numel()].view(x.shape)
    return sigmoid


def test_probes_are_exp_to_rounding(amd):
    """alpha = fsub(1, expf(fmul(-sigma, delta))): expf is within 1 ulp of e <= 1, i.e. within u = 2^-24 (2 u at a 2-ulp expf); the
    rounding of the product moves the exponent by at most |x| u and e by |x| e u <= u / e < 0.37 u; the subtraction rounds once, <= u / 2:
    under 2 u in all, and the bound is 4 u absolute against float64 of the same fp32 inputs.
    sigmoid = fdiv(1, fadd(1, expf(-x))): the 1-ulp (2 u relative) error of e moves s by s^2 e 2u = s (1 - s) 2u <= u / 2, the addition
    and the division each round once, s u each: under 2.5 u, and the bound is 3 u absolute."""
    gen = torch.Generator().manual_seed(9)
    sigma = torch.cat([torch.exp(3.0 * torch.randn(4000, generator=gen)), torch.tensor([0.0, 1e-30, 1e-10, 0.5, 1e4, 1e30])])
    delta = torch.cat([torch.rand(4000, generator=gen) * 0.2, torch.tensor([4.0 / 63, 0.0, 1e10, 1e10, 4.0 / 63, 1e10])])
    got = device_alpha(amd)(sigma, delta)
    want = 1.0 - torch.exp(-sigma.double() * delta.double())
    err_alpha = float((got.double() - want).abs().max())
    assert got[4000].item() == 0.0 and got[4001].item() == 0.0 and got[4004].item() == 1.0 and got[4005].item() == 1.0
    x = torch.cat([torch.randn(3999, generator=gen) * 6.0, torch.tensor([0.0, -0.0, 100.0, -100.0, 88.0, -88.0, 17.0])])
    got_s = device_sigmoid(amd)(x)
    err_sig = float((got_s.double() - torch.sigmoid(x.double())).abs().max())
    assert got_s[3999].item() == 0.5 and got_s[4001].item() == 1.0 and got_s[4002].item() == 0.0
    RS.record("gpu/probes", {"alpha_max_abs_err": err_alpha, "alpha_allowed": 4 * U, "sigmoid_max_abs_err": err_sig, "sigmoid_allowed": 3 * U,
                             "alpha_err_in_u": err_alpha / U, "sigmoid_err_in_u": err_sig / U})
    print(f"probes: alpha {err_alpha / U:.3f} u, sigmoid {err_sig / U:.3f} u")
    assert err_alpha <= 4 * U and err_sig <= 3 * U


# ---- the sampler, bit for bit ----------------------------------------------------------------------------------------------------------
def sampler_inputs(ts, us):
    raw, fam = RS.sampler_rays()
    tab = RS.sampler_tables()
    return raw, tab["t"][ts], tab["u"][us], fam


@pytest.mark.parametrize("ts,us", STRIDES)
def test_sampler_is_the_restatement_on_every_ray(amd, ts, us):
    raw, t, u, _ = sampler_inputs(ts, us)
    n, ustride = RS.N_EDGE, RS.u_stride(us)
    assert bool(torch.isnan(raw[:, :, :3]).all())                     # the kernels must not read the colours
    alpha_of = device_alpha(amd)
    sig = raw[:, :, 3].contiguous()
    rawd, td, ud = raw.cuda(), t.cuda(), u.cuda()
    want = RS.sample_fine(sig, t, u, alpha_of)
    ok = []
    for with_fine in (True, False):
        merged, fine = Guarded((n, 192), fill=NAN), Guarded((n, 128), fill=NAN)
        amd._lib.call("nerf_sample_fine_rays", rawd, td, ts, ud, ustride, n, merged.view, fine.view if with_fine else None, None, 0.0, 0.0)
        ok.append(same(merged.view, want["t_sorted"], f"rays: t_sorted (t {ts}, u {us})") and merged.intact() and fine.intact())
        if with_fine:
            ok.append(same(fine.view, want["t_fine"], f"rays: t_fine (t {ts}, u {us})"))
        else:
            ok.append(bool(torch.isnan(fine.view).all()))
    if ts == 0 and ustride == 0:
        for masks in (None,) + RS.MASK_THRESHOLDS:
            wantm = RS.sample_fine(sig, t, u, alpha_of, masks=masks)
            merged, fine, valid = Guarded((n, 192), fill=NAN), Guarded((n, 128), fill=NAN), GuardedBytes((n, 192))
            thr = masks or (0.0, 0.0)
            amd._lib.call("nerf_sample_fine", rawd, td, ud, n, merged.view, fine.view, valid.view if masks else None, thr[0], thr[1])
            ok.append(same(merged.view, wantm["t_sorted"], f"t_sorted (u {us}, masks {masks})") and merged.intact())
            ok.append(same(fine.view, wantm["t_fine"], f"t_fine (u {us}, masks {masks})") and fine.intact())
            if masks:
                ok.append(same(valid.view.float(), wantm["valid_sorted"].float(), f"valid_sorted (u {us}, masks {masks})"))
                both = Guarded((n, 192), fill=NAN), GuardedBytes((n, 192))
                amd._lib.call("nerf_sample_fine_rays", rawd, td, 0, ud, 0, n, both[0].view, None, both[1].view, thr[0], thr[1])
                ok.append(same(both[0].view, wantm["t_sorted"], "rays entry, shared tables") and torch.equal(both[1].view, valid.view))
            ok.append(valid.intact())
    assert all(ok), ok


# ---- compositing, bit for bit ----------------------------------------------------------------------------------------------------------
def composite_inputs(S, stride):
    raw, t, family = RS.composite_rays(S)
    return raw, (t[4].contiguous() if stride == 0 else t), family          # shared depths: the row with repeated depths


def offset_copy(t):
    """The same depths behind a pointer that is 4 bytes past a 16-byte boundary."""
    out = torch.empty(t.numel() + 1, device="cuda")[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize("S", RS.COMPOSITE_S + (193,))
def test_composite_is_the_restatement_on_every_ray(amd, S):
    alpha_of, sigmoid = device_alpha(amd), device_sigmoid(amd)
    ok = []
    for stride in (0, S):
        raw, t, _ = composite_inputs(S, stride)
        for white in (0, 1):
            want = RS.composite(raw, t, white, alpha_of, sigmoid)
            for n in RS.COMPOSITE_N:
                idx = RS.subset(n)
                rawd = raw[idx].contiguous().cuda()
                t_n = (t if stride == 0 else t[idx].contiguous()).cuda()
                depths = [t_n] + ([offset_copy(t_n)] if S % 16 == 0 else [])          # staged kernel, then the simple one
                for td in depths:
                    for with_w in (True, False):
                        rgb, dep, w = Guarded((n, 3), fill=NAN), Guarded((n,), fill=NAN), Guarded((n, S), fill=NAN)
                        amd._lib.call("nerf_composite", rawd, td, stride, n, S, white, rgb.view, dep.view, w.view if with_w else None)
                        what = f"S {S} n {n} white {white} stride {stride} aligned {td.data_ptr() % 16 == 0}"
                        ok.append(same(rgb.view, want[0][idx], "rgb, " + what) and rgb.intact())
                        ok.append(same(dep.view, want[1][idx], "depth, " + what) and dep.intact())
                        ok.append((same(w.view, want[2][idx], "weights, " + what) if with_w else bool(torch.isnan(w.view).all()))
                                  and w.intact())
    assert all(ok), f"{ok.count(False)} of {len(ok)} comparisons differ"


# ---- the adjoints ----------------------------------------------------------------------------------------------------------------------
def by_family(names, member, hip, f64, cpu32, what, figures, failures):
    """RS.rule per family of rays for one output tensor; keeps the figures of the family's worst case."""
    for name in names:
        rows = member(name)
        if not bool(rows.any()):
            continue
        measured, allowed, zero_ok = RS.rule(hip[rows], f64[rows], cpu32[rows])
        key = f"{what[0]}/{name}"
        worst = figures.get(key)
        if worst is None or measured * worst["allowed"] > worst["measured"] * allowed or (allowed == 0 and measured > 0):
            figures[key] = {"measured": measured, "allowed": allowed, "case": what[1]}
        if not zero_ok or measured > allowed:
            print(f"OVER {key} [{what[1]}]: measured {measured:.3e} allowed {allowed:.3e} zero rows exact {zero_ok}")
            failures.append((key, what[1], measured, allowed, zero_ok))


@pytest.mark.parametrize("S", RS.COMPOSITE_S)
def test_composite_adjoint(amd, S):
    alpha_of = device_alpha(amd)
    gen = torch.Generator().manual_seed(600 + S)
    N = RS.N_EDGE
    g_rgb, g_dep = torch.randn(N, 3, generator=gen), torch.randn(N, generator=gen)
    figures, failures = {}, []
    for stride in (0, S):
        raw, t, family = composite_inputs(S, stride)
        for white in (0, 1):
            twins = {gd: {dt: RS.composite_twin(raw, t, white, g_rgb, g_dep if gd else None, dt, alpha_of)
                          for dt in (torch.float64, torch.float32)} for gd in (True, False)}
            for n in RS.COMPOSITE_N:
                idx = RS.subset(n)
                rawd, gr, gdd = raw[idx].contiguous().cuda(), g_rgb[idx].contiguous().cuda(), g_dep[idx].contiguous().cuda()
                t_n = (t if stride == 0 else t[idx].contiguous()).cuda()
                for gd in (True, False):
                    for gt in (True, False):
                        if n != N and not (gd and gt):
                            continue
                        g_raw, g_t = Guarded((n + 1, S, 4), fill=NAN), Guarded((n + 1, S), fill=NAN)
                        amd._lib.call("nerf_composite_backward", rawd, t_n, stride, n, S, white, gr, gdd if gd else None, g_raw.view,
                                      g_t.view if gt else None)
                        hip_raw, hip_t = g_raw.view.cpu(), g_t.view.cpu()
                        case = f"S {S} n {n} white {white} stride {stride} g_depth {gd} g_t {gt}"
                        # exact contracts: nothing outside the n rows, rows of sigma <= 0 are zero, finite everywhere
                        assert g_raw.intact() and g_t.intact(), case
                        assert bool(torch.isnan(hip_raw[n]).all()) and bool(torch.isnan(hip_t[n:] if gt else hip_t).all()), case
                        assert bool(torch.isfinite(hip_raw[:n]).all()) and (not gt or bool(torch.isfinite(hip_t[:n]).all())), case
                        assert bool((hip_raw[:n][raw[idx][:, :, 3] <= 0] == 0).all()), case
                        member = lambda name: family[idx] == RS.COMPOSITE_FAMILIES.index(name)          # noqa: E731
                        f64, c32 = twins[gd][torch.float64], twins[gd][torch.float32]
                        by_family(RS.COMPOSITE_FAMILIES, member, hip_raw[:n], f64[0][idx], c32[0][idx], ("g_raw", case), figures, failures)
                        if gt:
                            by_family(RS.COMPOSITE_FAMILIES, member, hip_t[:n], f64[1][idx], c32[1][idx], ("g_t", case), figures, failures)
    RS.record(f"gpu/composite_adjoint/S{S}", figures)
    assert not failures, failures


def test_composite_adjoint_refuses_193_samples(amd):
    raw, t, _ = RS.composite_rays(193)
    g_raw = Guarded((1, 193, 4), fill=NAN)
    with pytest.raises(amd._lib.NerfLibraryError, match="192"):
        amd._lib.call("nerf_composite_backward", raw[:1].contiguous().cuda(), t[:1].contiguous().cuda(), 193, 1, 193, 1,
                      torch.ones(1, 3, device="cuda"), None, g_raw.view, None)
    assert bool(torch.isnan(g_raw.view).all()) and g_raw.intact()


@pytest.mark.parametrize("ts,us", STRIDES)
def test_sampler_adjoint(amd, ts, us):
    raw, t, u, fam = sampler_inputs(ts, us)
    n, ustride = RS.N_EDGE, RS.u_stride(us)
    sig = raw[:, :, 3].contiguous()
    dec = RS.sample_fine(sig, t, u, device_alpha(amd))
    G = torch.randn(n, 192, generator=torch.Generator().manual_seed(700))
    f64, c32 = (RS.sample_twin(sig, t, u, G, dt, dec) for dt in (torch.float64, torch.float32))
    rawd, td, ud, Gd = raw.cuda(), t.cuda(), u.cuda(), G.cuda()
    t_sorted = dec["t_sorted"].cuda()
    entries = [("nerf_sample_fine_rays_backward", (rawd, td, ts, ud, ustride, n, t_sorted, Gd))]
    if ts == 0 and ustride == 0:
        entries.append(("nerf_sample_fine_backward", (rawd, td, ud, n, t_sorted, Gd)))
    figures, failures = {}, []
    for entry, args in entries:
        g_raw = Guarded((n + 1, 64, 4), fill=NAN)
        amd._lib.call(entry, *args, g_raw.view)
        hip = g_raw.view.cpu()
        assert g_raw.intact() and bool(torch.isnan(hip[n]).all()), entry
        assert bool((hip[:n, :, :3] == 0).all()) and bool(torch.isfinite(hip[:n, :, 3]).all()), entry
        assert bool((hip[:n, :, 3][sig <= 0] == 0).all()), entry
        member = lambda name: torch.isin(torch.arange(n), torch.tensor(fam[name]))          # noqa: E731
        by_family(sorted(fam), member, hip[:n, :, 3], f64, c32, ("g_sigma", f"{entry} t {ts} u {us}"), figures, failures)
    RS.record(f"gpu/sampler_adjoint/t{ts}_u{us}", figures)
    assert not failures, failures
