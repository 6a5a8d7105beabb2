"""No GPU: the fused clip + Adam step's restatement (tests/adam_reference.py) against float64, against torch.optim.Adam behind
clip_grad_value_ on the CPU, and against seeded wrong variants of itself.

The bounds are those of adam_reference's docstring, derived per quantity from the count of roundings (u = 2^-24): m' carries the
roundings of the difference, of w1 and of the product, each of a term no larger than w1 |g - m|, plus the rounding of the sum; v' is a
sum of positives with two roundings in v*b2, three in (g*g)*w2 and one of the sum; p' carries u |p'| plus the propagated errors of m',
of the denominator (sqrt, bc2s, quotient, eps, sum) and the roundings of s, of the quotient and of the product.  None is measured.  They
hold where no intermediate is denormal, which the test checks of every family it applies them to.

torch on the CPU is bit-equal to the restatement at step 1 from zero state in m', and in v' once the restatement groups addcmul_'s
products as torch's CPU kernel does ((w2*g)*g; the device kernels and nerf_adam_step compute (g*g)*w2, adam_reference's docstring).
Two of torch's CPU kernels fuse a multiply-add that shows even at step 1: lerp_ for a weight >= 0.5 (beta1 <= 0.5) and add(p, alpha=wd)
(weight decay); in those hyper-parameter sets the affected quantity is held to its float64 bound instead.  Later
steps are held to the float64 bounds, in units of them; the ratios go to profiles/adam_parity.json."""
import numpy as np
import pytest
import torch

import adam_reference as R

F = np.float32
CASES = [(name, step) for name in R.HYPERS for step in R.STEPS]


def _bounded(fam):
    return fam.finite and fam.normal


@pytest.fixture(scope="module")
def edge_set():
    """{(hyper name, step): families}, built once."""
    return {(name, step): R.families(R.HYPERS[name], step) for name, step in CASES}


def test_restatement_is_within_the_float64_bounds(edge_set):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for (name, step), fams in edge_set.items():
        h = R.HYPERS[name]
        for fam in fams:
            if not _bounded(fam):
                continue
            assert not R.has_denormal(fam, h, step), (name, step, fam.name)
            got = R.adam_step_f32(fam.p, fam.g, fam.m, fam.v, h, step)
            q = R.ratios(got, R.adam_step_f64(fam.p, fam.g, fam.m, fam.v, h, step), h)
            for k in worst:
                worst[k] = max(worst[k], q[k])
            assert max(q.values()) <= 1.0, (name, step, fam.name, q)
    print("restatement / bound", worst)
    R.record("restatement_vs_f64", {k: round(x, 4) for k, x in worst.items()})


def test_every_family_reaches_its_branch(edge_set):
    names = set()
    for (name, step), fams in edge_set.items():
        for fam in fams:
            what, ok = R.reaches(fam, R.HYPERS[name], step)
            assert ok, (name, step, fam.name, what)
            assert fam.normal or fam.name.startswith("tiny_g")
            names.add(fam.name)
    assert len(names) == 12
    # the denormal families do produce denormals (without weight decay), so the device's handling of them is compared
    for name in ("nerf", "hashfield"):
        fams = {fam.name: fam for fam in edge_set[(name, 10)]}
        assert R.has_denormal(fams["tiny_g_v0"], R.HYPERS[name], 10) and R.has_denormal(fams["tiny_g_vpos"], R.HYPERS[name], 10)


def _torch_step(p, g, m, v, h, step):
    """clip_grad_value_ + one torch.optim.Adam step on the CPU from state (m, v, step - 1) -> (p', m', v') float32 arrays."""
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g.copy())
    opt = torch.optim.Adam([tp], lr=h.lr, betas=h.betas, eps=h.eps, weight_decay=h.weight_decay)
    opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    if h.clip > 0:
        torch.nn.utils.clip_grad_value_([tp], h.clip)
    opt.step()
    st = opt.state[tp]
    assert float(st["step"]) == step
    return tp.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()


@pytest.mark.parametrize("name", list(R.HYPERS))
def test_step_one_from_zero_state_is_torch_bit_for_bit(edge_set, name):
    h = R.HYPERS[name]
    p, g, _, _ = R.concat([fam for fam in edge_set[(name, 1)] if fam.finite])
    z = np.zeros_like(p)
    _, tm, tv = _torch_step(p, g, z, z, h, 1)
    _, m1, _ = R.adam_step_f32(p, g, z, z, h, 1)
    _, _, v1 = R.adam_step_f32(p, g, z, z, h, 1, cpu_grouping=True)
    x = R.adam_step_f64(p, g, z, z, h, 1)
    b = R.bounds(x, h)
    if h.weight_decay == 0:
        assert R.same_bits(tv, v1)
    else:                                      # torch's CPU add(p, alpha=wd) is one fused multiply-add: one rounding fewer in g
        normal = x["g2"] ** 2 * x["w2"] > 4 * R.TINY
        assert (np.abs(tv.astype(np.float64) - x["v1"]) <= b["v"])[normal].all() and normal.sum() > 2000
    if h.betas[0] > 0.5 and h.weight_decay == 0:
        assert R.same_bits(tm, m1)
    else:                                      # likewise its vectorised lerp for a weight >= 0.5: (w - 1) * (g - m) + g, fused
        assert (np.abs(tm.astype(np.float64) - x["m1"]) <= b["m"]).all()


def test_torch_over_six_steps_is_within_the_same_bounds():
    """Each of torch's steps is compared with adam_step_f64 of torch's own state before it; so is the restatement's, which carries
    its own state.  Gradients alternate between needing the clip and not, the learning rate moves."""
    worst = {"torch": {"p": 0.0, "m": 0.0, "v": 0.0}, "restatement": {"p": 0.0, "m": 0.0, "v": 0.0}}
    for name in ("nerf", "hashfield", "decay"):
        h0 = R.HYPERS[name]
        rng = np.random.default_rng(7)
        n = 4099
        p = rng.normal(size=n).astype(F)
        tstate = (p.copy(), np.zeros(n, F), np.zeros(n, F))
        rstate = (p.copy(), np.zeros(n, F), np.zeros(n, F))
        for step in range(1, 7):
            h = h0._replace(lr=h0.lr * 0.1 ** ((step - 1) * 40 / 500))
            g = (rng.normal(size=n) * (100.0 if step % 2 == 0 else 0.01)).astype(F)
            for who, state in (("torch", tstate), ("restatement", rstate)):
                x = R.adam_step_f64(state[0], g, state[1], state[2], h, step)
                new = _torch_step(*state[:1], g, *state[1:], h, step) if who == "torch" else R.adam_step_f32(state[0], g, state[1], state[2], h, step)
                q = R.ratios(new, x, h)
                assert max(q.values()) <= 1.0, (who, name, step, q)
                for k in q:
                    worst[who][k] = max(worst[who][k], q[k])
                if who == "torch":
                    tstate = new
                else:
                    rstate = new
    print("six steps, error / bound", worst)
    R.record("torch_cpu_vs_f64", {k: round(x, 4) for k, x in worst["torch"].items()})
    R.record("restatement_six_steps_vs_f64", {k: round(x, 4) for k, x in worst["restatement"].items()})


def test_nan_and_inf_gradients_give_what_torch_gives():
    h = R.HYPERS["nerf"]
    g = np.array([np.nan, np.inf, -np.inf, 100.0, -3.0], F)
    assert R.same_bits(R.clamp(g, F(40)), torch.from_numpy(g.copy()).clamp_(-40.0, 40.0).numpy())
    assert R.same_bits(R.clamp(g, F(40)), np.array([np.nan, 40, -40, 40, -3], F))
    p = np.array([0.5, -0.25, 1.0, 2.0, -1.0], F)
    z = np.zeros(5, F)
    tp, tm, tv = _torch_step(p, g, z, z, h, 1)
    rp, rm, rv = R.adam_step_f32(p, g, z, z, h, 1)
    _, _, rv_cpu = R.adam_step_f32(p, g, z, z, h, 1, cpu_grouping=True)
    assert np.isnan(tp[0]) and np.isfinite(tp[1:]).all()
    assert np.array_equal(np.isnan(rp), np.isnan(tp)) and R.same_bits(rm, tm) and R.same_bits(rv_cpu, tv)
    x = R.adam_step_f64(p[1:], g[1:], z[1:], z[1:], h, 1)
    assert (np.abs(tp[1:] - x["p1"]) <= R.bounds(x, h)["p"]).all() and (np.abs(rp[1:] - x["p1"]) <= R.bounds(x, h)["p"]).all()
    # the whole inf / NaN family, with the clip off too, where an infinite gradient is not tamed
    for name in ("nerf", "noclip"):
        h = R.HYPERS[name]
        fam = [f for f in R.families(h, 2) if f.name == "inf_nan"][0]
        tp, tm, tv = _torch_step(fam.p, fam.g, fam.m, fam.v, h, 2)
        rp, rm, rv = R.adam_step_f32(fam.p, fam.g, fam.m, fam.v, h, 2)
        for a, b in ((tp, rp), (tm, rm), (tv, rv)):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_seeded_wrong_variant_is_caught(edge_set, variant):
    """Every variant changes a compared bit on the edge set; every one but the NaN-swallowing clip and the parent's constants also
    leaves its float64 bound; the parent's constants leave the bound of v' at betas (0.9, 0.999)."""
    bits, bound = 0, {"p": 0, "m": 0, "v": 0}
    v_nerf, worst_nerf = 0, {"p": 0.0, "m": 0.0, "v": 0.0}
    for (name, step), fams in edge_set.items():
        h = R.HYPERS[name]
        for fam in fams:
            right = R.adam_step_f32(fam.p, fam.g, fam.m, fam.v, h, step)
            wrong = R.adam_step_f32(fam.p, fam.g, fam.m, fam.v, h, step, variant=variant)
            bits += sum(not R.same_bits(a, b) for a, b in zip(right, wrong))
            if _bounded(fam):
                x = R.adam_step_f64(fam.p, fam.g, fam.m, fam.v, h, step)
                b = R.bounds(x, h)
                for k, arr in zip("pmv", wrong):
                    with np.errstate(all="ignore"):
                        over = int((~(np.abs(arr.astype(np.float64) - x[k + "1"]) <= b[k])).sum())
                    bound[k] += over
                    if k == "v" and name == "nerf":
                        v_nerf += over
                if name == "nerf" and variant == "parent_constants":
                    q = R.ratios(wrong, x, h)
                    worst_nerf = {k: max(worst_nerf[k], q[k]) for k in q}
    print(variant, "outputs with changed bits", bits, "elements over the bound", bound)
    assert bits > 0
    if variant == "parent_constants":
        assert v_nerf > 0
        print("the parent's constants at betas (0.9, 0.999), error / bound", worst_nerf)
        R.record("parent_constants_vs_f64_at_nerf_hyper", {k: round(x, 2) for k, x in worst_nerf.items()})
    elif variant != "fmax_clip":
        assert sum(bound.values()) > 0
