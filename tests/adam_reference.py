"""Restatement of the fused clip + Adam step (include/nerf_mi355x.h: nerf_adam_step), in numpy on the CPU: the yardstick of
tests/test_adam_reference_cpu.py and tests/test_gpu_adam.py.  A helper, not a test; written from the header's formulas, and it imports
nothing of the package.

    adam_step_f32   one step in float32, every operation one separately rounded numpy operation (IEEE: correctly rounded sqrt and
                    division, denormals kept), in the kernel's order, with the constants formed as torch forms them from Python doubles
                    and rounded to fp32 once.  The kernel must equal it bit for bit.
    adam_step_f64   the same step in float64 from the same fp32 p, g, m, v and the double hyper-parameters, with the per-element
                    magnitudes of every intermediate.
    bounds          how far a float32 evaluation may lie from adam_step_f64, per quantity, from the count of roundings alone.
    families        the edge set: small vectors (p, g, m, v), each with the branch it is meant to reach (`reaches`).
    HYPERS, STEPS   the hyper-parameter sets and step counts the edge set is run at.

`variant` names one deliberately wrong step (tests of discrimination only), VARIANTS below.

Operation order.  It is that of torch's device kernels: addcmul_ as v*b2 + (g*g)*w2 and addcdiv_ as p + s*(m/denom).  torch's CPU kernels
group two products the other way -- (w2*g)*g and (s*m)/denom -- and fuse the multiply-add of lerp_; `cpu_grouping=True` restates the
first, which is all that is visible at step 1 from zero state, where the CPU comparison is bit for bit.

The bounds (u = 2^-24; every fp32 operation and every rounding of a constant has relative error <= u; no denormal intermediate).  E_x
is the bound of quantity x, |.| taken of the float64 values; clamp is 1-Lipschitz, so a clipped gradient inherits the rounding of clip.

    g2 = clamp(g) + wd*p    E_g = [|g| > clip] u clip + [wd != 0] (2u |wd p| + u |g2|)          (wd, the product; the sum)
    m' = m + (g2 - m)*w1    E_m = w1 E_g + 3u w1 |g2 - m| + u |m'|                              (the difference, w1, the product; the sum)
       = g2 - (g2 - m)*c    E_m = (1 + c) E_g + u (w1 + 2c) |g2 - m| + u |m'|                   (w1 >= 0.5, c = 1 - w1: fsub(1, w1) is exact,
                                                                                                 so c carries w1's rounding, absolute u w1)
    v' = v*b2 + (g2*g2)*w2  E_v = 2u b2 v + 3u w2 g2^2 + 2 w2 |g2| E_g + u v'                   (b2, product; square, w2, product; the sum)
    denom = sqrt(v')/bc2s + eps
                            E_d = (E_v / (2 sqrt v') + u sqrt v') / bc2s + 2u sqrt(v')/bc2s + u eps + u denom
                                                                                                (sqrt; bc2s, the quotient; eps; the sum)
    r = m'/denom            E_r = E_m / denom + |r| E_d / denom + u |r|
    p' = p + s*r            E_p = |s| E_r + 2u |s r| + u |p'|                                   (s, the product; the sum)

Each is multiplied by 1 + 2^-12 for the products of two first-order terms (each term is below 2^-19 relative).  Nothing here is measured."""
import json
import os
import shutil
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -12
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(REPO, "profiles", "adam_parity.json")
F = np.float32
TINY = float(np.finfo(np.float32).tiny)          # 2^-126: the smallest normal fp32

Hyper = namedtuple("Hyper", "lr betas eps weight_decay clip")
HYPERS = {
    "nerf": Hyper(5e-4, (0.9, 0.999), 1e-8, 0.0, 40.0),
    "hashfield": Hyper(1e-2, (0.9, 0.99), 1e-15, 0.0, 40.0),
    "decay": Hyper(5e-4, (0.9, 0.999), 1e-8, 1e-4, 40.0),
    "noclip": Hyper(5e-4, (0.9, 0.999), 1e-8, 0.0, 0.0),
    "scheduled": Hyper(5e-4 * 0.1 ** (137 / 500), (0.9, 0.999), 1e-8, 0.0, 40.0),      # FusedAdam.exponential_lr(5e-4, 137)
    "beta1_0.4": Hyper(5e-4, (0.4, 0.999), 1e-8, 0.0, 40.0),                           # lerp's other form (weight >= 0.5)
    "beta1_0": Hyper(5e-4, (0.0, 0.999), 1e-8, 0.0, 40.0),
}
STEPS = (1, 2, 10, 1000, 100000)
VARIANTS = ("eps_in_sqrt", "eps_before_div", "bc2_not_sqrt", "no_bc1", "step_minus_1", "w_beta1", "clip_after_wd", "v_unclipped",
            "p_old_m", "fmax_clip", "parent_constants")


def constants(h, step, variant=None):
    """The fp32 constants of one step -> dict(w1, b2, w2, bc2s, s, eps, wd, clip), formed in double and rounded once."""
    b1, b2 = h.betas
    with np.errstate(all="ignore"):
        if variant == "parent_constants":      # the kernel before this restatement: fp32 betas, 1 - beta and lr / bc1 formed in fp32
            bc1 = F(1.0 - float(F(b1)) ** step)
            return dict(w1=F(1) - F(b1), b2=F(b2), w2=F(1) - F(b2), bc2s=F(np.sqrt(1.0 - float(F(b2)) ** step)),
                        s=-(F(h.lr) / bc1), eps=F(h.eps), wd=F(h.weight_decay), clip=F(h.clip))
        k = step - 1 if variant == "step_minus_1" else step
        bc1 = np.float64(1.0) if variant == "no_bc1" else np.float64(1.0 - b1 ** k)
        bc2 = np.float64(1.0 - b2 ** k)
        return dict(w1=F(b1 if variant == "w_beta1" else 1.0 - b1), b2=F(b2), w2=F(1.0 - b2),
                    bc2s=F(bc2 if variant == "bc2_not_sqrt" else np.sqrt(bc2)), s=F(-(np.float64(h.lr) / bc1)),
                    eps=F(h.eps), wd=F(h.weight_decay), clip=F(h.clip))


def clamp(g, clip, variant=None):
    """clamp_(-clip, clip) as two comparisons: NaN passes, +-inf becomes +-clip."""
    if variant == "fmax_clip":
        return np.fmin(np.fmax(g, -clip), clip)
    g = g.copy()
    g[g < -clip] = -clip
    g[g > clip] = clip
    return g


def adam_step_f32(p, g, m, v, h, step, variant=None, cpu_grouping=False, trace=None):
    """(p, g, m, v) float32 arrays -> (p', m', v') float32.  trace: a dict that receives every intermediate."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == F
    c = constants(h, step, variant)
    with np.errstate(all="ignore"):
        g_raw = g
        if variant != "clip_after_wd" and c["clip"] > 0:
            g = clamp(g, c["clip"], variant)
        if c["wd"] != 0:
            wp = c["wd"] * p
            g = g + wp
            if variant == "v_unclipped":
                g_raw = g_raw + wp
        if variant == "clip_after_wd" and c["clip"] > 0:
            g = clamp(g, c["clip"])
        d = g - m
        if c["w1"] < F(0.5):
            t = d * c["w1"]
            m1 = m + t
        else:
            t = d * (F(1) - c["w1"])
            m1 = g - t
        gv = g_raw if variant == "v_unclipped" else g
        a = v * c["b2"]
        if cpu_grouping:
            q = c["w2"] * gv
            r2 = q * gv
        else:
            q = gv * gv
            r2 = q * c["w2"]
        v1 = a + r2
        if variant == "eps_in_sqrt":
            sq = np.sqrt(v1 + c["eps"])
            dv = sq / c["bc2s"]
            denom = dv
        elif variant == "eps_before_div":
            sq = np.sqrt(v1)
            dv = sq + c["eps"]
            denom = dv / c["bc2s"]
        else:
            sq = np.sqrt(v1)
            dv = sq / c["bc2s"]
            denom = dv + c["eps"]
        r = (m if variant == "p_old_m" else m1) / denom
        upd = c["s"] * r
        p1 = p + upd
    if trace is not None:
        trace.update(g2=g, d=d, t=t, a=a, q=q, r2=r2, sq=sq, dv=dv, denom=denom, r=r, upd=upd, m1=m1, v1=v1, p1=p1)
    return p1.astype(F), m1.astype(F), v1.astype(F)


def adam_step_f64(p, g, m, v, h, step):
    """The same step in float64 from fp32 inputs and the double hyper-parameters -> dict of float64 arrays: p1, m1, v1 and the
    intermediates g2, d (= g2 - m), sq (= sqrt v1), denom, r (= m1 / denom), upd (= s r), clipped (bool), and the scalars w1, b2, w2,
    bc2s, s."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == F
    p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
    b1, b2 = h.betas
    w1, w2 = 1.0 - b1, 1.0 - b2
    bc2s = np.sqrt(1.0 - b2 ** step)
    s = -(h.lr / (1.0 - b1 ** step))
    with np.errstate(all="ignore"):
        clipped = (np.abs(g) > h.clip) if h.clip > 0 else np.zeros(g.shape, bool)
        g2 = clamp(g, h.clip) if h.clip > 0 else g
        g2 = g2 + h.weight_decay * p if h.weight_decay != 0 else g2
        d = g2 - m
        m1 = m + d * w1 if w1 < 0.5 else g2 - d * (1.0 - w1)
        v1 = v * b2 + (g2 * g2) * w2
        sq = np.sqrt(v1)
        denom = sq / bc2s + h.eps
        r = m1 / denom
        upd = s * r
        p1 = p + upd
    return dict(p1=p1, m1=m1, v1=v1, g2=g2, d=d, sq=sq, denom=denom, r=r, upd=upd, clipped=clipped, p=p, v=v,
                w1=w1, b2=b2, w2=w2, bc2s=bc2s, s=s)


def bounds(x, h):
    """x = adam_step_f64(...) -> dict(p=E_p, m=E_m, v=E_v): the module docstring's bounds, per element."""
    wd, w1, w2 = h.weight_decay, x["w1"], x["w2"]
    with np.errstate(all="ignore"):
        e_g = np.where(x["clipped"], U * h.clip, 0.0)
        if wd != 0:
            e_g = e_g + 2 * U * np.abs(wd * x["p"]) + U * np.abs(x["g2"])
        ad = np.abs(x["d"])
        if w1 < 0.5:
            e_m = w1 * e_g + 3 * U * w1 * ad + U * np.abs(x["m1"])
        else:
            c = 1.0 - w1
            e_m = (1 + c) * e_g + U * (w1 + 2 * c) * ad + U * np.abs(x["m1"])
        e_v = 2 * U * x["b2"] * x["v"] + 3 * U * w2 * x["g2"] ** 2 + 2 * w2 * np.abs(x["g2"]) * e_g + U * x["v1"]
        half = np.where(x["v1"] > 0, e_v / (2 * np.where(x["v1"] > 0, x["sq"], 1.0)), 0.0)
        e_d = (half + U * x["sq"]) / x["bc2s"] + 2 * U * x["sq"] / x["bc2s"] + U * h.eps + U * x["denom"]
        e_r = e_m / x["denom"] + np.abs(x["r"]) * e_d / x["denom"] + U * np.abs(x["r"])
        e_p = abs(x["s"]) * e_r + 2 * U * np.abs(x["upd"]) + U * np.abs(x["p1"])
    return dict(p=SLACK * e_p, m=SLACK * e_m, v=SLACK * e_v)


def ratios(got, x, h):
    """got = (p', m', v') of some float32 evaluation, x = adam_step_f64 of the same inputs -> {quantity: worst |got - f64| / bound}
    (0 / 0 counts as 0: an exact result under a zero bound)."""
    b = bounds(x, h)
    out = {}
    for key, arr in zip("pmv", got):
        err = np.abs(arr.astype(np.float64) - x[key + "1"])
        with np.errstate(all="ignore"):
            q = np.where(err == 0, 0.0, err / b[key])
        assert not np.isnan(q).any(), key
        out[key] = float(q.max()) if q.size else 0.0
    return out


def same_bits(a, b):
    """Bit equality, NaN compared by position (any NaN equals any NaN; -0.0 differs from 0.0)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


# ---- the edge set ----------------------------------------------------------------------------------------------------------------------
Family = namedtuple("Family", "name p g m v finite normal")          # finite: no NaN / inf anywhere; normal: no denormal intermediate
N = 256


def log_uniform(rng, lo, hi, n=N):
    return (10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)) * rng.choice([-1.0, 1.0], n)


def families(h, step):
    """The edge set at hyper-parameters h and step `step` (two families place p by the step's own update) -> list of Family."""
    rng = np.random.default_rng(20240607)
    clip = h.clip if h.clip > 0 else 40.0
    f = lambda x: np.asarray(x, np.float64).astype(F)
    state = lambda: (f(rng.normal(size=N)), f(log_uniform(rng, 1e-6, 1.0)), f(log_uniform(rng, 1e-6, 1.0) ** 2))
    out = []
    p, m, v = state()
    out.append(Family("loguniform", p, f(log_uniform(rng, 1e-8, 1e2)), m, v, True, True))
    p, m, v = state()
    c = F(clip)
    edge = np.array([c, np.nextafter(c, F(np.inf)), np.nextafter(c, F(0))], F)
    out.append(Family("clip_edges", p, np.tile(np.concatenate([edge, -edge]), N // 6 + 1)[:N], m, v, True, True))
    p, m, v = state()
    out.append(Family("inf_nan", p, np.tile(np.array([np.inf, -np.inf, np.nan], F), N // 3 + 1)[:N], m, v, False, True))
    p = f(rng.normal(size=N))
    p[::4], p[1::4] = F(-0.0), F(0.0)
    z = np.zeros(N, F)
    g = z.copy()
    g[2::8] = F(-0.0)
    out.append(Family("untouched_rows", p, g, z.copy(), z.copy(), True, True))
    p, m, v = state()
    out.append(Family("tiny_g_v0", p, f(log_uniform(rng, 1e-25, 1e-19)), z.copy(), z.copy(), True, False))
    out.append(Family("tiny_g_vpos", p.copy(), f(log_uniform(rng, 1e-25, 1e-19)), m, v, True, False))
    p, m, v = state()
    out.append(Family("m_opposes_g", p, f(-m.astype(np.float64) * (1 + rng.uniform(-1e-6, 1e-6, N))), m, v, True, True))
    out.append(Family("m_equals_g", p.copy(), f(m.astype(np.float64) * (1 + rng.uniform(-1e-6, 1e-6, N))), m.copy(), v.copy(), True, True))
    p, _, _ = state()
    out.append(Family("v_large_m_tiny", p, f(log_uniform(rng, 1e-12, 1e-9)), f(log_uniform(rng, 1e-12, 1e-9)), f(log_uniform(rng, 1e2, 1e4) ** 2), True, True))
    out.append(Family("m_large_v_tiny", p.copy(), f(log_uniform(rng, 1e-9, 1e-7)), f(log_uniform(rng, 1.0, 30.0)), f(log_uniform(rng, 1e-10, 1e-8) ** 2), True, True))
    # p placed by the step's own update: -update (the sum cancels), and so large that the update is below half an ulp
    g, m, v = f(rng.normal(size=N)), f(0.1 * rng.normal(size=N)), f(1e-3 * rng.uniform(0.5, 2.0, N))
    p = z.copy()
    for _ in range(2):                         # (with weight decay the update depends on p: one refinement)
        p = f(-adam_step_f64(p, g, m, v, h, step)["upd"])
    p[1::3] = np.nextafter(p[1::3], F(np.inf))
    p[2::3] = np.nextafter(p[2::3], F(-np.inf))
    out.append(Family("p_cancels", p, g, m, v, True, True))
    big = f(1e4 * rng.uniform(1.0, 2.0, N) * rng.choice([-1.0, 1.0], N))
    for _ in range(3):
        upd = np.abs(adam_step_f64(big, g, m, v, h, step)["upd"])
        big = f(np.sign(big) * np.maximum(np.abs(big), 2.0 ** 27 * upd))
    out.append(Family("p_large", big, g.copy(), m.copy(), v.copy(), True, True))
    return out


def reaches(fam, h, step):
    """Does the family reach the branch it is meant to?  -> (description, bool), from the fp32 restatement's own intermediates."""
    tr = {}
    p1, m1, v1 = adam_step_f32(fam.p, fam.g, fam.m, fam.v, h, step, trace=tr)
    denormal = lambda x: (x != 0) & (np.abs(x) < TINY)
    clip = F(h.clip)
    name = fam.name
    if name == "loguniform":
        share = np.mean(np.abs(fam.g) > 40.0)
        return "gradients on both sides of the clip, seven decades below it", bool(0 < share < 1 and np.abs(fam.g).min() < 1e-7)
    if name == "clip_edges":
        if h.clip <= 0:
            return "clip off: every gradient passes unchanged", bool(h.weight_decay != 0 or np.array_equal(tr["g2"], fam.g))
        above = np.abs(fam.g) > clip
        ok = above.any() and (np.abs(fam.g) == clip).any() and (np.abs(fam.g) < clip).any()
        return "|g| at, above and below clip; exactly those above are moved", bool(ok and (h.weight_decay != 0 or np.array_equal(tr["g2"] != fam.g, above)))
    if name == "inf_nan":
        nan = np.isnan(fam.g)
        ok = np.array_equal(np.isnan(p1), nan) if h.clip > 0 else bool(np.isnan(p1).all())
        return "NaN gradients give NaN parameters; with a clip, infinite ones give finite parameters", bool(ok and np.isnan(m1[nan]).all() and np.isnan(v1[nan]).all())
    if name == "untouched_rows":
        if h.weight_decay != 0:
            return "weight decay moves even a row without gradient", bool((p1 != fam.p)[fam.p != 0].all())
        return "m = v = g = 0: p, m, v keep their bytes", bool(same_bits(p1, fam.p) and same_bits(m1, fam.m) and same_bits(v1, fam.v) and
                                                                 (np.signbit(fam.p) & (fam.p == 0)).any())
    if name in ("tiny_g_v0", "tiny_g_vpos"):
        q = tr["q"]
        if h.weight_decay != 0:
            return "weight decay lifts the gradient out of the underflow range", True
        return "g*g is denormal or zero everywhere, both occur", bool(((q == 0) | denormal(q)).all() and (q == 0).any() and denormal(q).any())
    if name == "m_opposes_g":
        return "g = -m to 1e-6", bool((np.sign(fam.g) == -np.sign(fam.m)).all() and (np.abs(fam.g + fam.m) <= 2e-6 * np.abs(fam.m)).all())
    if name == "m_equals_g":
        return "g - m cancels to 1e-6 of m", bool((np.abs(fam.g - fam.m) <= 2e-6 * np.abs(fam.m)).all())
    if name == "v_large_m_tiny":
        lim = 1e-10 if h.weight_decay == 0 else 1e-5            # (weight decay adds wd * p to the tiny gradient)
        return "|m / denom| below %g" % lim, bool((np.abs(tr["r"]) < lim).all())
    if name == "m_large_v_tiny":
        if h.betas[0] == 0:
            return "beta1 = 0: m' is the gradient whatever m was", bool(np.array_equal(m1, tr["g2"]))
        lim = 1e5 if h.weight_decay == 0 else 1e3               # (weight decay adds (wd * p)^2 * w2 to the tiny v)
        return "|m / denom| above %g" % lim, bool((np.abs(tr["r"]) > lim).all())
    if name == "p_cancels":
        return "the update cancels p to 2^-18 of it", bool((np.abs(p1) <= 2.0 ** -18 * np.abs(fam.p)).all() and (p1 != fam.p).all())
    if name == "p_large":
        return "the update is below half an ulp: p' == p", bool(same_bits(p1, fam.p) and (tr["upd"] != 0).all() and (np.abs(fam.p) >= 1e4).all())
    raise KeyError(name)


def has_denormal(fam, h, step):
    """Is any intermediate of the fp32 restatement denormal?"""
    tr = {}
    adam_step_f32(fam.p, fam.g, fam.m, fam.v, h, step, trace=tr)
    return any(bool(((x != 0) & (np.abs(x) < TINY)).any()) for x in tr.values())


def concat(fams):
    """The families of one (h, step) as one vector each -> (p, g, m, v)."""
    return tuple(np.concatenate([getattr(fm, k) for fm in fams]) for k in "pgmv")


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def record(key, stats):
    """Keep measured figures: merged into profiles/adam_parity.json under `key` (ray_side_reference.record's convention, its copy
    directory included)."""
    rec = {}
    if os.path.exists(PARITY_JSON):
        with open(PARITY_JSON) as fh:
            rec = json.load(fh)
    rec[key] = stats
    os.makedirs(os.path.dirname(PARITY_JSON), exist_ok=True)
    with open(PARITY_JSON, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
    out = os.environ.get("NERF_PARITY_COPY_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        shutil.copyfile(PARITY_JSON, os.path.join(out, os.path.basename(PARITY_JSON)))
