"""-m gpu: nerf_adam_step (the fused clip + Adam step, the last kernel of every training step) against its restatement
tests/adam_reference.py, bit for bit: p', m' and v' of every element must be the restatement's float32 values, NaN compared by position,
no element exempt.  Every buffer handed to the entry is the interior of a sentinel-filled one, the sentinels must be intact afterwards
and the gradient buffer unchanged.

    the edge set        every family of adam_reference.families at every hyper-parameter set and step count, one call per (set, step);
                        single tensors of 1, 63, 64, 65, 255, 256, 257 elements
    six steps           the kernel carries its own state under a moving learning rate, every step compared
    tensor boundaries   48 tensors in one call, zero-element ones first, in the middle and last, one of 2^20 + 513 elements that is not
                        the last (the grid of 4096 x 256 threads wraps, and the wrapped range crosses tensor ends), with 16-byte aligned
                        bases and with bases one float off; the refusals (49 tensors, step 0, a null pointer) write nothing
    power               the kernel's own outputs differ from every seeded wrong variant of the restatement
    FusedAdam           parameter groups, grad = None, mixed steps, non-contiguous gradients and parameters, NaN, untouched table rows
    float64             the kernel's worst error / bound per quantity on the denormal-free finite families (adam_reference's bounds, derived
                        from the count of roundings) is asserted <= 1 and kept in profiles/adam_parity.json next to torch's own."""
import numpy as np
import pytest
import torch

import adam_reference as R
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0x7FC0DEAD           # a quiet NaN with a payload no arithmetic produces
PAD = 64                        # floats on either side: the interior keeps the allocation's alignment; 65 puts it one float off 16 bytes
CASES = [(name, step) for name in R.HYPERS for step in R.STEPS]


class Guarded:
    """A device float buffer of `data` between two runs of sentinels; .t is the interior, the tensor the entry gets."""

    def __init__(self, data, pad=PAD):
        data = np.ascontiguousarray(data, F).reshape(-1)
        self.pad, self.n = pad, data.size
        if self.n == 0:             # an empty device tensor as torch makes it: its data pointer is null
            self.buf = self.t = torch.empty(0, device="cuda")
            assert self.t.data_ptr() == 0
            return
        host = torch.full((self.n + 2 * pad,), SENTINEL, dtype=torch.int32)
        host[pad:pad + self.n] = torch.from_numpy(data.view(np.int32).copy())
        self.buf = host.cuda().view(torch.float32)
        self.t = self.buf[pad:pad + self.n]
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (4 * pad) % 16

    def read(self):
        return self.t.cpu().numpy().copy()

    def intact(self):
        if self.n == 0:
            return True
        ints = self.buf.view(torch.int32).cpu()
        return bool((ints[:self.pad] == SENTINEL).all() and (ints[self.pad + self.n:] == SENTINEL).all())


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, F).view(np.int32), np.asarray(b, F).view(np.int32))


def _launch(L, rows, h, step):
    """rows: per tensor [p, g, m, v] as Guarded -> one nerf_adam_step over them."""
    cols = [[row[k].t for row in rows] for k in range(4)]
    L.call("nerf_adam_step", len(rows), *cols, [row[0].n for row in rows], h.lr, h.betas[0], h.betas[1], h.eps, h.weight_decay,
           h.clip, step)
    torch.cuda.synchronize()


def _step(L, items, h, step, pad=PAD):
    """items: per tensor (p, g, m, v) numpy arrays -> per tensor (p', m', v') from one call; sentinels and gradients checked."""
    rows = [[Guarded(a, pad) for a in item] for item in items]
    _launch(L, rows, h, step)
    out = []
    for row, item in zip(rows, items):
        assert all(x.intact() for x in row), "a sentinel next to a buffer was overwritten"
        assert _bits_equal(row[1].read(), item[1]), "the gradient buffer changed"
        out.append((row[0].read(), row[2].read(), row[3].read()))
    return out


def _assert_same(got, want, what):
    """Bit equality of (p', m', v') with the restatement's; the message names the first differing elements."""
    for key, a, b in zip("pmv", got, want):
        if not R.same_bits(a, b):
            bad = np.flatnonzero(~((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))
            raise AssertionError(f"{what}: {key}' differs in {bad.size} of {a.size} elements, first at {bad[:5].tolist()}: "
                                 f"kernel {a[bad[:5]].tolist()} restatement {b[bad[:5]].tolist()}")


_edge_cache = {}


def _edge(L, name, step):
    """The kernel's output on the edge set at (name, step): (families, inputs, outputs), computed once per module run."""
    if (name, step) not in _edge_cache:
        h = R.HYPERS[name]
        fams = R.families(h, step)
        inputs = R.concat(fams)
        _edge_cache[(name, step)] = (fams, inputs, _step(L, [inputs], h, step)[0])
    return _edge_cache[(name, step)]


@pytest.mark.parametrize("name,step", CASES)
def test_edge_set_is_the_restatement_bit_for_bit(amd, name, step):
    h = R.HYPERS[name]
    fams, (p, g, m, v), got = _edge(amd._lib, name, step)
    want = R.adam_step_f32(p, g, m, v, h, step)
    off = 0
    for fam in fams:                                            # family by family, so that a mismatch names its family
        sl = slice(off, off + fam.p.size)
        _assert_same([x[sl] for x in got], [x[sl] for x in want], f"{name} step {step} {fam.name}")
        off += fam.p.size
    assert off == p.size


@pytest.mark.parametrize("pad", [PAD, PAD + 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_one_tensor_of_n_elements(amd, n, pad):
    rng = np.random.default_rng(n)
    for name in ("nerf", "hashfield"):
        h = R.HYPERS[name]
        item = (rng.normal(size=n).astype(F), (R.log_uniform(rng, 1e-8, 1e2, n)).astype(F), (0.1 * rng.normal(size=n)).astype(F),
                (rng.uniform(0, 1e-2, n)).astype(F))
        _assert_same(_step(amd._lib, [item], h, 3, pad)[0], R.adam_step_f32(*item, h, 3), f"{name} n {n}")


def test_six_consecutive_steps_carry_the_kernels_own_state(amd):
    h0 = R.HYPERS["decay"]
    rng = np.random.default_rng(3)
    sizes = [256 * 63, 256, 128 * 283, 3 * 128, 1]
    state = [(rng.normal(size=n).astype(F), np.zeros(n, F), np.zeros(n, F)) for n in sizes]          # the restatement's p, m, v
    rows = [[Guarded(p), None, Guarded(m), Guarded(v)] for p, m, v in state]
    for step in range(1, 7):
        h = h0._replace(lr=h0.lr * 0.1 ** ((step - 1) * 40 / 500))
        grads = [(rng.normal(size=n) * (100.0 if step % 2 == 0 else 0.01)).astype(F) for n in sizes]     # every other step needs the clip
        for row, g in zip(rows, grads):
            row[1] = Guarded(g)
        _launch(amd._lib, rows, h, step)
        state = [R.adam_step_f32(p, g, m, v, h, step) for (p, m, v), g in zip(state, grads)]
        for i, (row, want, g) in enumerate(zip(rows, state, grads)):
            assert all(x.intact() for x in row) and _bits_equal(row[1].read(), g)
            _assert_same((row[0].read(), row[2].read(), row[3].read()), want, f"step {step} tensor {i}")


BIG = (1 << 20) + 513
SIZES_48 = [0, 1, 255, 256, 257, 7, BIG, 3, 0, 63, 64, 65, 1000, 129, 0, 31] + [5 + 37 * i for i in range(31)] + [0]


def _boundary_items(seed=48):
    rng = np.random.default_rng(seed)
    n = sum(SIZES_48)
    flat = (rng.normal(size=n).astype(F), R.log_uniform(rng, 1e-8, 1e2, n).astype(F), (0.1 * rng.normal(size=n)).astype(F),
            rng.uniform(0, 1e-2, n).astype(F))
    ends = np.cumsum(SIZES_48)
    return flat, [tuple(a[e - s:e] for a in flat) for s, e in zip(SIZES_48, ends)]


@pytest.mark.parametrize("pad", [PAD, PAD + 1])
def test_forty_eight_tensors_across_the_grid_stride_wrap(amd, pad):
    assert len(SIZES_48) == 48 and SIZES_48[0] == SIZES_48[8] == SIZES_48[-1] == 0 and SIZES_48.index(BIG) < 47
    assert sum(SIZES_48[:6]) < 4096 * 256 < sum(SIZES_48[:7])          # the wrap begins inside the big tensor and runs over all later ones
    h = R.HYPERS["hashfield"]
    flat, items = _boundary_items()
    got = _step(amd._lib, items, h, 3, pad)
    want = R.adam_step_f32(*flat, h, 3)
    off = 0
    for i, (n, out) in enumerate(zip(SIZES_48, got)):
        _assert_same(out, [x[off:off + n] for x in want], f"tensor {i} of {n} elements")
        off += n


def test_refusals_write_nothing(amd):
    L = amd._lib
    h = R.HYPERS["nerf"]
    rng = np.random.default_rng(49)
    items = [tuple(rng.normal(size=4).astype(F) for _ in range(4)) for _ in range(49)]
    rows = [[Guarded(a) for a in item] for item in items]

    def refused(rows, step, text, numel=None, null=None):
        cols = [[row[k].t for row in rows] for k in range(4)]
        if null is not None:
            cols[null[0]][null[1]] = None
        with pytest.raises(L.NerfLibraryError) as info:
            L.call("nerf_adam_step", len(rows), *cols, numel or [row[0].n for row in rows], h.lr, *h.betas, h.eps, h.weight_decay, h.clip, step)
        assert "nerf_adam_step" in str(info.value) and "status -1" in str(info.value) and text in str(info.value)

    refused(rows, 1, "bad size")                                   # a 49th tensor
    refused(rows[:3], 0, "bad size")                               # step 0
    refused(rows[:3], 1, "bad size", numel=[4, -1, 4])
    for k in range(4):                                             # a null pointer of a tensor with elements, in each of the four arrays
        refused(rows[:3], 1, "null tensor", null=(k, 1))
    torch.cuda.synchronize()
    for row, item in zip(rows, items):
        assert all(x.intact() and _bits_equal(x.read(), a) for x, a in zip(row, item))
    # the same null pointers with numel 0 are stepped over: the entry does not examine them, and the neighbours are stepped
    cols = [[rows[0][k].t, None, rows[2][k].t] for k in range(4)]
    L.call("nerf_adam_step", 3, *cols, [4, 0, 4], h.lr, *h.betas, h.eps, h.weight_decay, h.clip, 1)
    torch.cuda.synchronize()
    for i in (0, 2):
        _assert_same((rows[i][0].read(), rows[i][2].read(), rows[i][3].read()), R.adam_step_f32(*items[i], h, 1), f"tensor {i}")
        assert all(x.intact() for x in rows[i])


def test_the_kernel_fails_every_seeded_wrong_restatement(amd):
    """The power of the bit comparison on the device: against each wrong variant the kernel's own output differs somewhere in the edge
    set (at the second step of every hyper-parameter set, which is where all of them show)."""
    caught = {}
    for name in R.HYPERS:
        h = R.HYPERS[name]
        _, (p, g, m, v), got = _edge(amd._lib, name, 2)
        for variant in R.VARIANTS:
            wrong = R.adam_step_f32(p, g, m, v, h, 2, variant=variant)
            caught[variant] = caught.get(variant, 0) + sum(int((~((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b)))).sum())
                                                           for a, b in zip(got, wrong))
    print("elements that differ from each wrong variant", caught)
    assert all(caught[variant] > 0 for variant in R.VARIANTS), caught
    R.record("kernel_vs_wrong_variants_differing_elements", caught)


def test_the_kernel_is_within_the_float64_bounds(amd):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for name, step in CASES:
        h = R.HYPERS[name]
        fams, _, got = _edge(amd._lib, name, step)
        off = 0
        for fam in fams:
            sl = slice(off, off + fam.p.size)
            off += fam.p.size
            if fam.finite and fam.normal:
                q = R.ratios([x[sl] for x in got], R.adam_step_f64(fam.p, fam.g, fam.m, fam.v, h, step), h)
                assert max(q.values()) <= 1.0, (name, step, fam.name, q)
                worst = {k: max(worst[k], q[k]) for k in worst}
    print("kernel error / bound", worst)
    R.record("kernel_vs_f64", {k: round(x, 4) for k, x in worst.items()})


# ---- FusedAdam -------------------------------------------------------------------------------------------------------------------------
def _param(a):
    return torch.nn.Parameter(torch.from_numpy(np.array(a, F)).cuda())


def _np(t):
    return t.detach().cpu().numpy().copy()


def _opt_state(opt, p):
    st = opt.state[p]
    return _np(p), _np(st["exp_avg"]), _np(st["exp_avg_sq"])


def test_fused_adam_two_parameter_groups(amd):
    from nerf_replication_amd.training import FusedAdam
    rng = np.random.default_rng(11)
    ha, hb = R.HYPERS["decay"], R.Hyper(1e-2, (0.8, 0.99), 1e-15, 0.0, 0.5)
    shapes = [(33, 7), (257,)], [(64, 2), (1,), (5, 5, 5)]
    host = [[rng.normal(size=s).astype(F) for s in grp] for grp in shapes]
    params = [[_param(a) for a in grp] for grp in host]
    opt = FusedAdam([dict(params=params[0], lr=ha.lr, betas=ha.betas, eps=ha.eps, weight_decay=ha.weight_decay, clip_value=ha.clip),
                     dict(params=params[1], lr=hb.lr, betas=hb.betas, eps=hb.eps, weight_decay=hb.weight_decay, clip_value=hb.clip)])
    state = [[(a.reshape(-1), np.zeros(a.size, F), np.zeros(a.size, F)) for a in grp] for grp in host]
    for step in (1, 2, 3):
        for grp, sgrp, h in zip(params, state, (ha, hb)):
            for i, p in enumerate(grp):
                g = (rng.normal(size=tuple(p.shape)) * (3.0 if step == 2 else 0.1)).astype(F)
                p.grad = torch.from_numpy(g).cuda()
                sgrp[i] = R.adam_step_f32(sgrp[i][0], g.reshape(-1), sgrp[i][1], sgrp[i][2], h, step)
        opt.step()
        for grp, sgrp in zip(params, state):
            for i, p in enumerate(grp):
                _assert_same([x.reshape(-1) for x in _opt_state(opt, p)], sgrp[i], f"step {step} tensor {i}")
                assert float(opt.state[p]["step"]) == step


def test_fused_adam_leaves_parameters_without_gradient_alone(amd):
    from nerf_replication_amd.training import FusedAdam
    rng = np.random.default_rng(12)
    h = R.HYPERS["nerf"]
    host = [rng.normal(size=n).astype(F) for n in (65, 3, 256, 17)]
    params = [_param(a) for a in host]
    opt = FusedAdam(params, lr=h.lr, betas=h.betas, eps=h.eps, weight_decay=h.weight_decay, clip_value=h.clip)
    grads = {0: rng.normal(size=65).astype(F), 2: rng.normal(size=256).astype(F)}
    for i, g in grads.items():
        params[i].grad = torch.from_numpy(g).cuda()
    opt.step()
    for i, p in enumerate(params):
        if i in grads:
            z = np.zeros(p.numel(), F)
            _assert_same(_opt_state(opt, p), R.adam_step_f32(host[i], grads[i], z, z, h, 1), f"tensor {i}")
        else:
            assert _bits_equal(_np(p), host[i]) and len(opt.state.get(p, {})) == 0
    # the mixed steps this leaves behind are refused as they were (per-tensor steps are not implemented), before anything is written
    for p in params:
        p.grad = torch.zeros_like(p)
    before = [_np(p) for p in params]
    with pytest.raises(ValueError, match="tensors of one group are at different steps"):
        opt.step()
    assert all(_bits_equal(_np(p), b) for p, b in zip(params, before))


def test_fused_adam_layouts_and_nan(amd):
    from nerf_replication_amd.training import FusedAdam
    rng = np.random.default_rng(13)
    h = R.HYPERS["nerf"]
    kw = dict(lr=h.lr, betas=h.betas, eps=h.eps, weight_decay=h.weight_decay, clip_value=h.clip)
    # a non-contiguous gradient gives the bytes of its contiguous copy
    a, g = rng.normal(size=(8, 16)).astype(F), rng.normal(size=(16, 8)).astype(F)
    p = _param(a)
    p.grad = torch.from_numpy(g).cuda().t()
    assert not p.grad.is_contiguous()
    opt = FusedAdam([p], **kw)
    opt.step()
    z = np.zeros(a.size, F)
    _assert_same([x.reshape(-1) for x in _opt_state(opt, p)], R.adam_step_f32(a.reshape(-1), np.ascontiguousarray(g.T).reshape(-1), z, z, h, 1), "transposed gradient")
    # a non-contiguous parameter is refused by name and argument, and keeps its bytes
    q = torch.nn.Parameter(torch.from_numpy(a).cuda().t())
    assert not q.is_contiguous()
    q.grad = torch.ones_like(q)
    opt = FusedAdam([q], **kw)
    with pytest.raises(amd._lib.NerfLibraryError) as info:
        opt.step()
    assert "nerf_adam_step" in str(info.value) and "argument 1" in str(info.value)
    assert _bits_equal(_np(q), np.ascontiguousarray(a.T))
    # after a NaN gradient the parameter is NaN (clip_grad_value_ is clamp_, which lets NaN through), its neighbours are stepped
    a = rng.normal(size=6).astype(F)
    g = np.array([1.0, np.nan, -1e3, np.inf, -np.inf, 0.0], F)
    p = _param(a)
    p.grad = torch.from_numpy(g).cuda()
    opt = FusedAdam([p], **kw)
    opt.step()
    got = _opt_state(opt, p)
    z = np.zeros(6, F)
    _assert_same(got, R.adam_step_f32(a, g, z, z, h, 1), "NaN gradient")
    assert np.isnan(got[0][1]) and np.isfinite(np.delete(got[0], 1)).all()


def test_fused_adam_keeps_the_bytes_of_untouched_table_rows(amd):
    """A hash table [2^14, 2] at eps = 1e-15: rows no sample touched have m = v = g = 0 and must keep their bytes, -0.0 included."""
    from nerf_replication_amd.training import FusedAdam
    rng = np.random.default_rng(14)
    h = R.HYPERS["hashfield"]
    rows = 1 << 14
    a = rng.uniform(-1e-4, 1e-4, size=(rows, 2)).astype(F)
    a[::7] = F(-0.0)
    a[1::7] = F(0.0)
    p = _param(a)
    opt = FusedAdam([p], lr=h.lr, betas=h.betas, eps=h.eps, weight_decay=h.weight_decay, clip_value=h.clip)
    never = np.ones(rows, bool)
    state = (a.reshape(-1), np.zeros(2 * rows, F), np.zeros(2 * rows, F))
    for step in (1, 2, 3):
        touched = rng.random(rows) < 0.2
        touched[:8] = False
        never &= ~touched
        g = np.where(touched[:, None], R.log_uniform(rng, 1e-9, 1e-2, 2 * rows).reshape(rows, 2), 0.0).astype(F)
        p.grad = torch.from_numpy(g).cuda()
        opt.step()
        state = R.adam_step_f32(state[0], g.reshape(-1), state[1], state[2], h, step)
        got = _opt_state(opt, p)
        _assert_same([x.reshape(-1) for x in got], state, f"step {step}")
        assert never.sum() > rows // 3 and _bits_equal(got[0][never], a[never])
        assert not got[1][never].any() and not got[2][never].any() and not np.signbit(got[1][never]).any()
