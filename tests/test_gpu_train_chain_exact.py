"""-m gpu: the training MLP pair held to torch.equal.  On the probe networks of tests/f16_reference.py, exact points and an integer
d loss / d raw, every row the SAVE forwards store (pe, dpe, h0..h7, feature, views, the ReLU sign-bit blocks, raw), every row the
data-gradient chains store (g_zv, g_f, g_z0..7), g_x, g_t, the direction adjoints and the 24 parameter gradients on their exact
columns are small multiples of 1/4 whose sums stay below 2^24 units in any order (tests/train_chain_reference.py, checked on the
CPU by tests/test_train_chain_reference_cpu.py): the f32 and the f32x pair must return the float64 result BIT FOR BIT.  No
tolerance and no exempt element, except the sin / cos columns of the two non-zero axes in pe / dpe (5e-7 / 2e-6) and the 22 528
weight-gradient elements that multiply them (not compared).  A mismatch is a wrong row, mask bit, join or scale in the kernel that
wrote the named tensor -- or, in a gradient alone, in its weight-gradient kernel; the message names the first (tensor, point, column).

`save` and `gsave` start as NaN; every buffer a call writes sits between sentinels that must survive it.  Rows >= P are not
compared (the pad32 padding may hold duplicates).  Cases, each for f32 and f32x on the coarse and the fine model: the full pair in
ray mode at P = 1, 31, 32, 33, 127, 129, 185 with a shared depth table and per-ray depths (also nerf_mlp_backward and the chain
alone: bit-identical rows); point mode at 33 and 185; the density-only pair at 33 and 160; the for-compositing forward with dead
tiles at 160 and 192; the masked pair at P = 160 with 70 and 96 compact rows; and per precision one call of 2 * 128 * CUs + 461
points.  The tallies and the file's run time go to profiles/train_chain_exact.json.

Measured on the MI355X (profiles/train_chain_exact.json): 380 calls, 7.8e8 values compared, no mismatch in either precision; against
a reference with any of the six seeded faults of train_chain_reference.FAULTS the same kernels fail; the file runs in about 4 s."""
import functools
import time

import pytest
import torch

import f16_reference as R
import train_chain_reference as T
from train_chain_reference import Grad, Save, pad32
from gpu_common import amd, network  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL, PAD = -77.0, 64                       # 256 bytes on either side: the alignment of a torch allocation is kept
NAN = float("nan")
PROBE_OF = {"": (0, 0), "fine": (1, 1)}         # the coarse and the fine sub-model are different probe networks
MANY_PROBE = (2, 2)
N_POOL = 1024
PE_TOL, DPE_TOL = 5e-7, 2e-6                    # the inexact encoding columns: tests/test_gpu_training.py's bounds
COLOUR = (16, 17, 18, 19, 22, 23)               # views_linears.0, feature_linear, rgb_linear

SAVE_REGIONS = [("pe", Save.off_pe, 64), ("dpe", Save.off_dpe, 32)] + [(f"h{l}", functools.partial(Save.off_h, l=l), 256) for l in range(8)] + \
               [("feature", Save.off_f, 256), ("views", Save.off_hv, 128)]
GRAD_REGIONS = [("gzv", Grad.off_gzv, 128), ("gf", Grad.off_gf, 256)] + [(f"gz{l}", functools.partial(Grad.off_gz, l=l), 256) for l in range(7, -1, -1)]
TRUNK_SAVE = ("pe",) + tuple(f"h{l}" for l in range(8))
TRUNK_GRAD = tuple(f"gz{l}" for l in range(8))

_record = {}
_t0 = [None]


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def _keep_the_figures():
    _t0[0] = time.time()
    yield
    if _record:
        total = dict(calls=sum(r["calls"] for r in _record.values()), values_compared=sum(r["values_compared"] for r in _record.values()),
                     points_compared=sum(r["points_compared"] for r in _record.values()), mismatches=sum(r["mismatches"] for r in _record.values()))
        T.exact_record("cases", dict(sorted(_record.items())))
        T.exact_record("total", total)
        T.exact_record("seconds_for_the_whole_file", round(time.time() - _t0[0], 1))


@pytest.fixture(autouse=True)
def _default_dead_tile_skipping(monkeypatch):
    monkeypatch.delenv("NERF_DEAD_TILE_SKIP", raising=False)


@functools.lru_cache(maxsize=None)
def _sub(probe):
    torch.set_num_threads(8)
    return R.probe_network(*probe)


@functools.lru_cache(maxsize=None)
def _network(precision, many):
    """One Network per precision: the two probe sub-models of PROBE_OF (many: MANY_PROBE as both)."""
    import nerf_replication_amd as pkg
    sd = R.both_models(_sub(MANY_PROBE)) if many else \
        {f"{m}.{k}": v.clone() for m, key in (("model", ""), ("model_fine", "fine")) for k, v in _sub(PROBE_OF[key]).items()}
    return network(pkg, sd, precision, train=False)


# ================================================================================ buffers and comparisons
class Buffers:
    """Every buffer a call may write, each between two sentinel pads."""

    def __init__(self):
        self.all = []

    def new(self, n, fill, dtype=torch.float32):
        whole = torch.full((n + 2 * PAD,), SENTINEL if dtype.is_floating_point else int(SENTINEL), dtype=dtype, device="cuda")
        inner = whole[PAD:PAD + n]
        inner.fill_(fill)
        self.all.append((whole, n))
        return inner

    def grads(self):
        return [self.new(int(torch.tensor(s).prod()), 0.0).view(s) for s in T.PARAM_SHAPES]

    def intact(self):
        return all(bool((w[:PAD] == SENTINEL).all() and (w[PAD + n:] == SENTINEL).all()) for w, n in self.all)


class Tally:
    def __init__(self, tag):
        self.tag, self.calls, self.values, self.points, self.mismatches, self.failures = tag, 0, 0, 0, 0, []

    def same(self, got, want, what, close=None, tol=0.0):
        """got == want as numbers, element by element (a NaN never is); `close`: bool per column, False where |got - want| <= tol is
        asked instead.  A mismatch is kept with its first (point, column), so that one run lists every call that disagrees."""
        got = got.reshape(want.shape[0], -1) if want.dim() > 1 else got.reshape(-1, 1)
        want = want.to(got.device).double().reshape(got.shape)
        self.values += got.numel()
        self.points += got.shape[0]
        bad = got.double() != want
        if close is not None:
            close = close.to(got.device)
            bad[:, ~close] = ~((got.double() - want).abs()[:, ~close] <= tol)
        if not bool(bad.any()):
            return
        p, c = bad.nonzero()[0].tolist()
        self.mismatches += int(bad.sum())
        self.failures.append(f"{self.tag} {what}: {int(bad.sum())} of {bad.numel()} values at {int(bad.any(-1).sum())} of {bad.shape[0]} points differ; "
                             f"first at (point {p}, column {c}): got {got[p, c].item()!r}, want {want[p, c].item()!r}")

    def note(self, ok, what):
        self.values += 1
        if not ok:
            self.mismatches += 1
            self.failures.append(f"{self.tag} {what}")

    def close(self):
        _record[self.tag] = dict(calls=self.calls, values_compared=self.values, points_compared=self.points, mismatches=self.mismatches)
        assert not self.failures, "\n".join(self.failures)


def _region(buf, off, P, ld):
    return buf[off(P):off(P) + pad32(P) * ld].view(pad32(P), ld)


def _check_rows(tally, buf, regions, names, P, ref, what, rows=None, zero_axis=None):
    """The rows < P (or `rows`, ascending buffer rows whose reference is ref[name][k] for the k-th of them) of the named regions."""
    for name, off, ld in regions:
        if name not in names:
            continue
        got = _region(buf, off, P, ld)
        got = got[:P] if rows is None else got[rows]
        close, tol = None, 0.0
        if name in ("pe", "dpe"):
            cols = T.exact_columns(zero_axis)
            close, tol = (cols[0], PE_TOL) if name == "pe" else (cols[1], DPE_TOL)
        tally.same(got, ref[name], f"{what} {name}", close, tol)


def _check_bits(tally, save, P, ref, what, density_only=False, tiles=None):
    n_tiles = pad32(P) // 32
    got = save[Save.off_bits(P):Save.off_bits(P) + n_tiles * 9 * 256].view(torch.int32).view(n_tiles, 9, 64, 4)
    want, compared = T.bits_blocks(ref, P, density_only)
    want, compared = want.to(got.device), compared.to(got.device)
    if tiles is not None:
        keep = torch.zeros(n_tiles, dtype=torch.bool, device=got.device)
        keep[torch.as_tensor(tiles, dtype=torch.long, device=got.device)] = True
        compared = compared & keep[:, None, None, None]
    bad = (got != want) & compared
    tally.values += int(compared.sum())
    if bool(bad.any()):
        t, which, lane, word = bad.nonzero()[0].tolist()
        tally.mismatches += int(bad.sum())
        tally.failures.append(f"{tally.tag} {what} sign bits: {int(bad.sum())} words differ; first at tile {t}, tensor {which} (0..7 = h0..h7, 8 = views), lane "
                              f"{lane} (point {32 * t + (lane & 31)}), word {word}: got {int(got[t, which, lane, word]) & 0xffffffff:#010x}, "
                              f"want {int(want[t, which, lane, word]) & 0xffffffff:#010x}")


def _check_grads(tally, grads, ref, masks, what, zero=()):
    T.check_conditions(ref, masks)                    # the any-order conditions of THIS case, before anything is compared
    for i, (g, want, keep) in enumerate(zip(grads, ref["grads"], masks)):
        if i in zero:
            tally.note(bool((g == 0).all()), f"{what} gradient {i} of the colour branch is not exactly zero")
            continue
        tally.note(bool(torch.isfinite(g).all()), f"{what} gradient {i} is not finite")
        keep = keep.to(g.device)
        bad = (g.double() != want.to(g.device)) & keep
        tally.values += int(keep.sum())
        if bool(bad.any()):
            idx = bad.nonzero()[0].tolist()
            tally.mismatches += int(bad.sum())
            tally.failures.append(f"{tally.tag} {what} gradient {i} ({T.oracle.SUBMODEL_KEYS[i]}): {int(bad.sum())} of {int(keep.sum())} exact elements differ; "
                                  f"first at {idx}: got {g[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}")


def _same_bits(tally, a, b, P, regions, names, what):
    """Bit-identical rows < P of two buffers (the header's promise for calls that differ in their optional outputs)."""
    for name, off, ld in regions:
        if name in names:
            x, y = _region(a, off, P, ld)[:P].view(torch.int32), _region(b, off, P, ld)[:P].view(torch.int32)
            tally.note(torch.equal(x, y), f"{what}: the {name} rows are not bit-identical")


def _live_count(gsave, P):
    return int(gsave.view(torch.int32)[Grad.off_count(P)].item())


def _all_names(regions):
    return tuple(n for n, _, _ in regions)


# ================================================================================ the calls
class Rays:
    """Ray-mode inputs on the device, and the forward / backward entries over them."""

    def __init__(self, amd, net, model, rc, draw, density_only=False):
        self.L, self.net, self.model, self.dens = amd._lib, net, model, density_only
        self.n, self.S, self.P = rc["n_rays"], rc["S"], rc["n_rays"] * rc["S"]
        self.o, self.d, self.t, self.stride = rc["o"].cuda().contiguous(), rc["d"].cuda().contiguous(), rc["t"].cuda().contiguous(), rc["stride"]
        self.prec = self.L.PRECISIONS[net.precision]
        self.buf = Buffers()
        self.draw = self.buf.new(pad32(self.P) * 4, NAN)
        self.draw[:self.P * 4] = draw.reshape(-1).cuda()
        self.rays = (self.o, self.d, self.t, self.stride, self.n, self.S)

    def forward(self, entry, raw_fill=NAN, extra=()):
        self.raw = self.buf.new(self.P * 4, raw_fill)
        self.save = self.buf.new(int(self.L.call("nerf_train_save_floats", self.P)), NAN)
        self.L.call(entry, *self.rays, *extra, self.net.packed(self.model), self.raw, self.save, self.prec)
        torch.cuda.synchronize()
        return self.raw.view(self.P, 4)

    def backward(self, g_t=True, g_x=True, grads=True, entry="nerf_mlp_backward_rays_x"):
        """-> (gsave, g_t, g_x, grads), each in fresh buffers"""
        gsave = self.buf.new(int(self.L.call("nerf_train_grad_floats", self.P)), NAN)
        gt = self.buf.new(self.P, NAN) if g_t else None
        gx = self.buf.new(self.P * 3, NAN) if g_x else None
        gr = self.buf.grads() if grads else None
        head = (*self.rays, self.net.packed_bwd(self.model), self.draw, self.save, gsave, gt)
        if entry == "nerf_mlp_backward_rays_x":
            self.L.call(entry, *head, gx, gr, 1 if self.dens else 0, self.prec)
        else:
            assert gx is None and gr is not None
            self.L.call(entry, *head, gr, self.prec)
        torch.cuda.synchronize()
        return gsave, gt, None if gx is None else gx.view(self.P, 3), gr

    def view_adjoint(self, gsave):
        out = self.buf.new(self.n * 3, NAN)
        w_views = self._sub().ordered_params()[16].detach().contiguous()
        self.L.call("nerf_rays_viewdirs_backward", self.d, self.n, self.S, gsave, w_views, out)
        torch.cuda.synchronize()
        return out.view(self.n, 3)

    def _sub(self):
        return self.net.model_fine if self.model == "fine" else self.net.model


@functools.lru_cache(maxsize=None)
def _ray_ref(probe, P, per_ray, density_only=False):
    seed, zero_axis = probe
    rc = T.ray_case(seed, zero_axis, *T.RAY_SHAPES[P], per_ray)
    draw = T.integer_draw(P, 100 * seed + P + (1 if per_ray else 0))
    ref = T.reference(_sub(probe), rc["pts"], rc["dirs"], draw, n_samples=rc["S"], rays_d=rc["d"], density_only=density_only)
    return rc, draw, ref


CASES = [(precision, model) for precision in ("f32", "f32x") for model in ("", "fine")]


# ================================================================================ 1: the full pair, ray mode
@pytest.mark.parametrize("precision,model", CASES)
def test_full_pair_ray_mode(amd, precision, model):
    probe = PROBE_OF[model]
    masks = T.exact_masks(probe[1])
    tally = Tally(f"full_pair_rays/{precision}/{model or 'coarse'}")
    net = _network(precision, False)
    for P in (1, 31, 32, 33, 127, 129, 185):
        for per_ray in (False, True):
            rc, draw, ref = _ray_ref(probe, P, per_ray)
            what = f"P={P} {'per-ray depths' if per_ray else 'shared depth table'}"
            run = Rays(amd, net, model, rc, draw)
            raw = run.forward("nerf_mlp_forward_rays_save")
            tally.same(raw, ref["raw"], f"{what} raw")
            _check_rows(tally, run.save, SAVE_REGIONS, _all_names(SAVE_REGIONS), P, ref, what, zero_axis=probe[1])
            _check_bits(tally, run.save, P, ref, what)
            gsave, g_t, g_x, grads = run.backward()
            _check_rows(tally, gsave, GRAD_REGIONS, _all_names(GRAD_REGIONS), P, ref, what)
            tally.same(g_x, ref["g_x"], f"{what} g_x")
            tally.same(g_t, ref["g_t"], f"{what} g_t")
            tally.same(run.view_adjoint(gsave), ref["g_rays_d_view"], f"{what} g_rays_d_view")
            _check_grads(tally, grads, ref, masks, what)
            want_count = T.tile_liveness(draw)[1] if P % 32 == 0 else -1
            tally.note(_live_count(gsave, P) == want_count, f"{what}: live count {_live_count(gsave, P)}, want {want_count}")
            # nerf_mlp_backward (no g_x) and the chain alone (grads == NULL): the same rows, bit for bit
            gsave_b, g_t_b, _, grads_b = run.backward(g_x=False, entry="nerf_mlp_backward")
            _same_bits(tally, gsave, gsave_b, P, GRAD_REGIONS, _all_names(GRAD_REGIONS), f"{what} nerf_mlp_backward against nerf_mlp_backward_rays_x")
            tally.note(torch.equal(g_t.view(torch.int32), g_t_b.view(torch.int32)), f"{what}: g_t of nerf_mlp_backward is not bit-identical")
            _check_grads(tally, grads_b, ref, masks, f"{what} nerf_mlp_backward")
            gsave_c, g_t_c, g_x_c, _ = run.backward(grads=False)
            _same_bits(tally, gsave, gsave_c, P, GRAD_REGIONS, _all_names(GRAD_REGIONS), f"{what} grads == NULL")
            tally.note(torch.equal(g_t.view(torch.int32), g_t_c.view(torch.int32)) and torch.equal(g_x.view(torch.int32), g_x_c.view(torch.int32)),
                       f"{what}: g_t / g_x of the grads == NULL call are not bit-identical")
            tally.note(run.buf.intact(), f"{what}: a sentinel around a buffer was overwritten")
            tally.calls += 5
    tally.close()


# ================================================================================ 2: point mode
@functools.lru_cache(maxsize=None)
def _point_ref(probe, P):
    seed, zero_axis = probe
    n, S = T.RAY_SHAPES[P]
    pts, dirs = R.probe_points(seed, zero_axis, P)
    dirs = dirs[:n].contiguous()                                     # one direction per ray, used as given (not unit length)
    draw = T.integer_draw(P, 300 * seed + P)
    ref = T.reference(_sub(probe), pts, dirs[:, None, :].expand(n, S, 3).reshape(P, 3), draw, n_samples=S)
    return pts, dirs, draw, ref


@pytest.mark.parametrize("precision,model", CASES)
def test_point_mode_pair(amd, precision, model):
    L, probe = amd._lib, PROBE_OF[model]
    masks = T.exact_masks(probe[1])
    tally = Tally(f"point_mode/{precision}/{model or 'coarse'}")
    net = _network(precision, False)
    prec = L.PRECISIONS[precision]
    w_views = (net.model_fine if model == "fine" else net.model).ordered_params()[16].detach().contiguous()
    for P in (33, 185):
        n, S = T.RAY_SHAPES[P]
        pts, dirs, draw, ref = _point_ref(probe, P)
        what = f"P={P}"
        buf = Buffers()
        pts_d, dirs_d = pts.cuda().contiguous(), dirs.cuda().contiguous()
        draw_d = buf.new(pad32(P) * 4, NAN)
        draw_d[:P * 4] = draw.reshape(-1).cuda()
        raw = buf.new(P * 4, NAN)
        save = buf.new(int(L.call("nerf_train_save_floats", P)), NAN)
        gsave = buf.new(int(L.call("nerf_train_grad_floats", P)), NAN)
        g_pts, g_dirs, grads = buf.new(P * 3, NAN), buf.new(n * 3, NAN), buf.grads()
        L.call("nerf_mlp_forward_points_save", pts_d, dirs_d, n, S, net.packed(model), raw, save, prec)
        L.call("nerf_mlp_backward_points", pts_d, n, S, net.packed_bwd(model), draw_d, save, gsave, g_pts, grads, prec)
        L.call("nerf_viewdirs_backward", gsave, n, S, w_views, dirs_d, g_dirs)
        torch.cuda.synchronize()
        tally.same(raw.view(P, 4), ref["raw"], f"{what} raw")
        _check_rows(tally, save, SAVE_REGIONS, _all_names(SAVE_REGIONS), P, ref, what, zero_axis=probe[1])
        _check_bits(tally, save, P, ref, what)
        _check_rows(tally, gsave, GRAD_REGIONS, _all_names(GRAD_REGIONS), P, ref, what)
        tally.same(g_pts.view(P, 3), ref["g_x"], f"{what} g_pts")
        tally.same(g_dirs.view(n, 3), ref["g_v"], f"{what} g_viewdirs")
        _check_grads(tally, grads, ref, masks, what)
        tally.note(buf.intact(), f"{what}: a sentinel around a buffer was overwritten")
        tally.calls += 3
    tally.close()


# ================================================================================ 3: the density-only pair
@pytest.mark.parametrize("precision,model", CASES)
def test_density_only_pair(amd, precision, model):
    """d loss / d raw keeps non-zero rgb columns: the density entries must not read them."""
    probe = PROBE_OF[model]
    masks = T.exact_masks(probe[1])
    tally = Tally(f"density_only/{precision}/{model or 'coarse'}")
    net = _network(precision, False)
    for P in (33, 160):
        rc, draw, ref = _ray_ref(probe, P, True, True)
        what = f"P={P}"
        run = Rays(amd, net, model, rc, draw, density_only=True)
        raw = run.forward("nerf_mlp_forward_rays_save_density")
        want_raw = ref["raw"].clone()
        want_raw[:, :3] = 0
        tally.same(raw, want_raw, f"{what} raw = (0, 0, 0, sigma)")
        _check_rows(tally, run.save, SAVE_REGIONS, TRUNK_SAVE, P, ref, what, zero_axis=probe[1])
        _check_bits(tally, run.save, P, ref, what, density_only=True)
        gsave, g_t, _, grads = run.backward(g_x=False, entry="nerf_mlp_backward_density")
        _check_rows(tally, gsave, GRAD_REGIONS, TRUNK_GRAD, P, ref, what)
        tally.same(g_t, ref["g_t"], f"{what} g_t")
        _check_grads(tally, grads, ref, masks, what, zero=COLOUR)
        gsave_x, g_t_x, g_x, _ = run.backward(grads=False)           # nerf_mlp_backward_rays_x(density_only = 1): the chain alone
        _same_bits(tally, gsave, gsave_x, P, GRAD_REGIONS, TRUNK_GRAD, f"{what} nerf_mlp_backward_rays_x(density_only)")
        tally.same(g_x, ref["g_x"], f"{what} g_x")
        tally.same(g_t_x, ref["g_t"], f"{what} g_t of nerf_mlp_backward_rays_x")
        want_count = T.tile_liveness(draw, True)[1] if P % 32 == 0 else -1
        tally.note(_live_count(gsave, P) == want_count, f"{what}: live count {_live_count(gsave, P)}, want {want_count}")
        tally.note(run.buf.intact(), f"{what}: a sentinel around a buffer was overwritten")
        tally.calls += 3
    tally.close()


# ================================================================================ 4: for compositing, with dead tiles
def _interleave(n_tiles, n_dead):
    """tile order: a live tile first, then dead and live ones in turn"""
    live, dead, out = list(range(n_dead, n_tiles)), list(range(n_dead)), []
    while live or dead:
        if live:
            out.append(live.pop(0))
        if dead:
            out.append(dead.pop(0))
    return out


@functools.lru_cache(maxsize=None)
def _pool(probe):
    """1024 one-sample rays of a probe network with per-ray depths, and sigma of each."""
    seed, zero_axis = probe
    rc = T.ray_case(seed, zero_axis, N_POOL, 1, True)
    sigma = T.forward(_sub(probe), rc["pts"], rc["dirs"])["raw"][:, 3]
    return rc, sigma


def _take(rc, ids):
    return dict(o=rc["o"][ids].contiguous(), d=rc["d"][ids].contiguous(), t=rc["t"][ids].contiguous(), stride=1, n_rays=len(ids), S=1,
                pts=rc["pts"][ids].contiguous(), dirs=rc["dirs"][ids].contiguous())


@functools.lru_cache(maxsize=None)
def _dead_tile_ref(probe, P, n_dead):
    pool, sigma = _pool(probe)
    n_tiles = P // 32
    ids = T.arrange_dead_tiles(sigma, P, n_dead).view(n_tiles, 32)[_interleave(n_tiles, n_dead)].reshape(-1)
    rc = _take(pool, ids)
    draw = T.integer_draw(P, 500 + P) * (sigma[ids] > 0)[:, None].float()      # the contract: zero wherever sigma <= 0
    ref = T.reference(_sub(probe), rc["pts"], rc["dirs"], draw, n_samples=1, rays_d=rc["d"])
    assert torch.equal(ref["raw"][:, 3], sigma[ids])
    dead = ~(ref["raw"][:, 3] > 0).view(n_tiles, 32).any(-1)
    assert int(dead.sum()) == n_dead and not bool(dead[0])
    return rc, draw, ref, dead


@pytest.mark.parametrize("precision,model", CASES)
def test_for_compositing_pair_with_dead_tiles(amd, precision, model):
    probe = PROBE_OF[model]
    masks = T.exact_masks(probe[1])
    tally = Tally(f"for_compositing_dead_tiles/{precision}/{model or 'coarse'}")
    net = _network(precision, False)
    for P, n_dead in ((160, 2), (192, 3)):
        rc, draw, ref, dead = _dead_tile_ref(probe, P, n_dead)
        flags, count = T.tile_liveness(draw)
        assert flags.tolist() == (~dead).tolist()                   # every tile with a sigma > 0 has a non-zero gradient row
        what = f"P={P} ({n_dead} dead tiles)"
        live_rows = (~dead).repeat_interleave(32).nonzero().flatten().cuda()
        dead_rows = dead.repeat_interleave(32).nonzero().flatten().cuda()
        live_ref = {k: v[live_rows.cpu()] for k, v in ref.items() if torch.is_tensor(v) and v.shape[0] == P}
        dead_ref = {k: v[dead_rows.cpu()] for k, v in ref.items() if torch.is_tensor(v) and v.shape[0] == P}
        run = Rays(amd, net, model, rc, draw)
        raw = run.forward("nerf_mlp_forward_rays_save_for_compositing")
        tally.same(raw[live_rows], live_ref["raw"], f"{what} raw of live tiles")
        want_dead = dead_ref["raw"].clone()
        want_dead[:, :3] = 0                                         # a tile without density stops after the sigma head: rgb = 0
        tally.same(raw[dead_rows], want_dead, f"{what} raw of dead tiles")
        _check_rows(tally, run.save, SAVE_REGIONS, _all_names(SAVE_REGIONS), P, live_ref, f"{what} live tiles", rows=live_rows, zero_axis=probe[1])
        # what both precisions store of a dead tile: everything up to its h6 row
        _check_rows(tally, run.save, SAVE_REGIONS, ("pe",) + tuple(f"h{l}" for l in range(7)), P, dead_ref, f"{what} dead tiles", rows=dead_rows,
                    zero_axis=probe[1])
        _check_bits(tally, run.save, P, ref, what, tiles=(~dead).nonzero().flatten().tolist())
        gsave, g_t, g_x, grads = run.backward()
        tally.note(_live_count(gsave, P) == count, f"{what}: live count {_live_count(gsave, P)}, want {count}")
        _check_rows(tally, gsave, GRAD_REGIONS, _all_names(GRAD_REGIONS), P, live_ref, f"{what} live tiles", rows=live_rows)
        tally.same(g_x[live_rows], live_ref["g_x"], f"{what} g_x of live tiles")
        tally.same(g_t[live_rows], live_ref["g_t"], f"{what} g_t of live tiles")
        tally.note(bool((g_x[dead_rows] == 0).all() and (g_t[dead_rows] == 0).all()), f"{what}: g_t / g_x of a dead tile is not exactly zero")
        tally.same(run.view_adjoint(gsave), ref["g_rays_d_view"], f"{what} g_rays_d_view")
        _check_grads(tally, grads, ref, masks, what)                 # (the reference's rows of dead points are zero: a sum over live points)
        tally.note(run.buf.intact(), f"{what}: a sentinel around a buffer was overwritten")
        tally.calls += 3
    tally.close()


# ================================================================================ 5: the masked pair
@functools.lru_cache(maxsize=None)
def _masked_ref(probe, P, M):
    seed, zero_axis = probe
    rc = T.ray_case(seed, zero_axis, *T.RAY_SHAPES[P], True)
    sigma = T.forward(_sub(probe), rc["pts"], rc["dirs"])["raw"][:, 3]
    for attempt in range(16):                                        # the first seeded list whose compact tiles all carry a gradient
        g = torch.Generator().manual_seed(700 + M + 1000 * attempt)
        ids = torch.sort(torch.randperm(P, generator=g)[:M]).values
        draw = T.integer_draw(P, 600 + M + 1000 * attempt)
        draw[ids] = draw[ids] * (sigma[ids] > 0)[:, None].float()    # listed rows: zero wherever sigma <= 0; unlisted rows are never read
        padded = torch.zeros(pad32(M), 4)
        padded[:M] = draw[ids]
        count = T.tile_liveness(padded)[1]
        if count == pad32(M) // 32:
            break
    assert count == pad32(M) // 32
    valid = torch.zeros(P, dtype=torch.uint8)
    valid[ids] = 1
    ref = T.reference(_sub(probe), rc["pts"][ids], rc["dirs"][ids], draw[ids], n_samples=1)
    d_pts = rc["d"][:, None, :].expand(rc["n_rays"], rc["S"], 3).reshape(P, 3)[ids].double()
    ref["g_t"] = (ref["g_x"] * d_pts).sum(-1)
    return rc, valid, ids, draw, ref, count


@pytest.mark.parametrize("precision,model", CASES)
def test_masked_pair(amd, precision, model):
    L, probe = amd._lib, PROBE_OF[model]
    masks = T.exact_masks(probe[1])
    tally = Tally(f"masked/{precision}/{model or 'coarse'}")
    net = _network(precision, False)
    P = 160
    for M in (70, 96):
        rc, valid, ids, draw, ref, count = _masked_ref(probe, P, M)
        what = f"P={P} M={M}"
        run = Rays(amd, net, model, rc, draw)
        index, n_listed = run.buf.new(P, -7, torch.int32), run.buf.new(1, -7, torch.int32)
        ws_c = torch.empty(int(L.call("nerf_compact_valid_workspace_bytes", P)), dtype=torch.uint8, device="cuda")
        L.call("nerf_compact_valid", valid.cuda(), P, index, n_listed, ws_c)
        raw = run.forward("nerf_mlp_forward_rays_save_masked", raw_fill=0.0, extra=(index, n_listed))
        tally.note(int(n_listed.item()) == M and index[:M].tolist() == ids.tolist(), f"{what}: nerf_compact_valid's list differs")
        ids_d = ids.cuda()
        unlisted = (valid == 0).nonzero().flatten().cuda()
        tally.same(raw[ids_d], ref["raw"], f"{what} raw at the global ids")
        tally.note(bool((raw[unlisted] == 0).all()), f"{what}: raw of an unlisted point was written")
        compact = torch.arange(M, device="cuda")
        _check_rows(tally, run.save, SAVE_REGIONS, _all_names(SAVE_REGIONS), P, ref, f"{what} compact", rows=compact, zero_axis=probe[1])
        got_bits = run.save[Save.off_bits(P):Save.off_bits(P) + (pad32(M) // 32) * 9 * 256].view(torch.int32).view(pad32(M) // 32, 9, 64, 4)
        want_bits, compared = T.bits_blocks(ref, M)
        bad = (got_bits != want_bits.cuda()) & compared.cuda()
        tally.values += int(compared.sum())
        tally.note(not bool(bad.any()), f"{what} sign bits: {int(bad.sum())} words differ, first at (tile, tensor, lane, word) "
                                        f"{bad.nonzero()[0].tolist() if bool(bad.any()) else None}")
        gsave = run.buf.new(int(L.call("nerf_train_grad_floats", P)), NAN)
        g_t, grads = run.buf.new(P, NAN), run.buf.grads()
        ws = run.buf.new(int(L.call("nerf_mlp_backward_masked_workspace_bytes", P)) // 4, 0.0)
        L.call("nerf_mlp_backward_masked", *run.rays, index, n_listed, net.packed_bwd(model), run.draw, run.save, gsave, g_t, grads, run.prec, ws)
        torch.cuda.synchronize()
        tally.note(_live_count(gsave, P) == count, f"{what}: live count {_live_count(gsave, P)}, want {count}")
        _check_rows(tally, gsave, GRAD_REGIONS, _all_names(GRAD_REGIONS), P, ref, f"{what} compact", rows=compact)
        tally.same(g_t[ids_d], ref["g_t"], f"{what} g_t at the global ids")
        tally.note(bool((g_t[unlisted] == 0).all()), f"{what}: g_t of an unlisted point is not exactly zero")
        _check_grads(tally, grads, ref, masks, what)
        tally.note(run.buf.intact(), f"{what}: a sentinel around a buffer was overwritten")
        tally.calls += 3
    tally.close()


# ================================================================================ 6: many tiles
@pytest.mark.parametrize("precision", ["f32", "f32x"])
def test_many_tiles(amd, cus, precision):
    """2 * 128 * CUs + 3 * 128 + 77 one-sample rays out of 1024 distinct ones: every persistent f32x workgroup walks two or three
    128-point tiles, the f32 pair runs thousands of one-wave workgroups, the last tile is ragged.  Rows, bits, g_x and g_t only."""
    P = T.n_many(cus)
    pool, _ = _pool(MANY_PROBE)
    pool_draw = T.integer_draw(N_POOL, 900)
    ref = T.reference(_sub(MANY_PROBE), pool["pts"], pool["dirs"], pool_draw, n_samples=1, rays_d=pool["d"])
    T.check_conditions(ref, [torch.zeros(s, dtype=torch.bool) for s in T.PARAM_SHAPES])       # (no gradient is compared)
    many = R.repeated(P, N_POOL, 11).cuda()
    on_dev = {k: v.cuda()[many] for k, v in ref.items() if torch.is_tensor(v) and v.shape[0] == N_POOL}
    tally = Tally(f"many_tiles/{precision}")
    net = _network(precision, True)
    rc = dict(o=pool["o"].cuda()[many], d=pool["d"].cuda()[many], t=pool["t"].cuda()[many], stride=1, n_rays=P, S=1)
    run = Rays(amd, net, "fine", rc, pool_draw.cuda()[many])
    what = f"P={P}"
    raw = run.forward("nerf_mlp_forward_rays_save")
    tally.same(raw, on_dev["raw"], f"{what} raw")
    _check_rows(tally, run.save, SAVE_REGIONS, _all_names(SAVE_REGIONS), P, on_dev, what, zero_axis=MANY_PROBE[1])
    _check_bits(tally, run.save, P, on_dev, what)
    gsave, g_t, g_x, _ = run.backward(grads=False)
    _check_rows(tally, gsave, GRAD_REGIONS, _all_names(GRAD_REGIONS), P, on_dev, what)
    tally.same(g_x, on_dev["g_x"], f"{what} g_x")
    tally.same(g_t, on_dev["g_t"], f"{what} g_t")
    tally.note(_live_count(gsave, P) == -1, f"{what}: a ragged point count ran with a live-tile list")
    tally.note(run.buf.intact(), f"{what}: a sentinel around a buffer was overwritten")
    tally.calls += 2
    tally.close()
