"""-m gpu: the weight-gradient kernels (csrc/nerf_wgrad_f32.hip.inc, nerf_wgrad_bf16x3.hip.inc, nerf_wgrad_table.h) per element, at the
smallest point counts at which each slice or ring edge of their work partitions exists.  tests/wgrad_reference.py has the layout,
the job list, the partitions and the bounds; tests/test_wgrad_reference_cpu.py checks that yardstick on the CPU.

  integer probes   nerf_wgrad on integers in [-8, 8] (and dz times 2^-20): every product and partial sum is an integer below 2^24, so
                   dW and db must be BIT-EQUAL to the integer product in any summation order; NaN in every column that exists in
                   memory but not in the layer; sentinels around dw and db; a second call gives exactly twice the product.  Every row
                   of the table, aligned and unaligned, in the plain, ring and single-job 256 x 256 ring forms.
  own operands     nerf_mlp_backward / _density / _masked, f32 and f32x: after the call, every one of the 14 (10) GEMMs is recomputed
                   in float64 from the rows the chain itself wrote (gsave), the forward saved (save) and the incoming gradient, and
                   every element of every gradient is held to the derived bound of its kernel family (wgrad_reference's docstring).
                   The chain's own error is not in the comparison.  Inputs: a gradient that is zero except on at most 8 marker rows
                   placed on the edges of the partition (a row that is dropped, duplicated or attributed to another point shows in
                   every element it touches), and a dense random one.
The worst error / bound ratio per kernel family and the run time of this file go to profiles/wgrad_bounds.json.

Measured on the MI355X (profiles/wgrad_bounds.json): every integer probe bit-equal; worst error / bound 0.32 for the bf16x3 dW, 0.45 - 0.52
for the fp32 families, 0.33 - 0.44 for db; the file runs in about 3 s."""
import time

import pytest
import torch

import wgrad_reference as R
from gpu_common import amd  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL, PAD = -77.0, 8
_worst = {}
_probes = {"calls_bit_equal": 0}
_t0 = [None]


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(scope="module")
def net(amd, synthetic_sd):
    n = amd.Network()
    n.load_state_dict(synthetic_sd, strict=True)
    return n.cuda().eval()


@pytest.fixture(scope="module", autouse=True)
def _keep_the_figures():
    _t0[0] = time.time()
    yield
    if _probes["calls_bit_equal"]:
        R.parity_record("integer_probes", dict(_probes))
    if _worst:
        R.parity_record("worst_error_over_bound", {k: round(v, 4) for k, v in sorted(_worst.items())})
        R.parity_record("seconds_for_the_whole_file", round(time.time() - _t0[0], 1))


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), ratio)


def _padded(n):
    whole = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    inner = whole[PAD:PAD + n]
    inner.zero_()
    return whole, inner


def _intact(whole, n):
    return bool((whole[:PAD] == SENTINEL).all() and (whole[PAD + n:] == SENTINEL).all())


# ================================================================================ 1: layout and coverage, with the device's own numbers
def test_layout_mirror_matches_the_library(amd):
    L = amd._lib
    for P in (1, 31, 32, 33, 185, 533, 2048, 2592, 16385):
        assert int(L.call("nerf_train_save_floats", P)) == R.Save.floats(P)
        assert int(L.call("nerf_train_grad_floats", P)) == R.Grad.floats(P)
        assert int(L.call("nerf_train_live_count_offset", P)) == R.Grad.off_count(P)


def test_cases_visit_every_regime_on_this_device(cus):
    from test_gpu_training import _SMALL_LAYOUTS, _WGRAD_ROW_SHAPES
    assert R.WGRAD_ROW_SHAPES == _WGRAD_ROW_SHAPES and R.SMALL_LAYOUTS == _SMALL_LAYOUTS
    R.check_coverage(cus)


# ================================================================================ 2: integer probes of nerf_wgrad
def _probe(amd, layout, P, scale, seed):
    L = amd._lib
    (ldz, zc0, n_out), (ldh, hc0, n_in), (ldw, wc0), bias = layout
    gen = torch.Generator(device="cuda").manual_seed(seed)
    dz_i = torch.randint(-R.PROBE_MAX, R.PROBE_MAX + 1, (P, n_out), device="cuda", generator=gen).double()
    hin_i = torch.randint(-R.PROBE_MAX, R.PROBE_MAX + 1, (P, n_in), device="cuda", generator=gen).double()
    dz = torch.full((P, ldz), float("nan"), device="cuda")
    hin = torch.full((P, ldh), float("nan"), device="cuda")
    dz[:, zc0:zc0 + n_out] = (dz_i * scale).float()
    hin[:, hc0:hc0 + n_in] = hin_i.float()
    want_w = ((dz_i.T @ hin_i) * scale)                       # integers below 2^24 times a power of two: exact in float64 and in fp32
    want_b = dz_i.sum(0) * scale
    assert torch.equal(want_w.float().double(), want_w) and torch.equal((2 * want_w).float().double(), 2 * want_w)
    whole_w, dw = _padded(n_out * ldw)
    whole_b, db = _padded(n_out)
    for call in (1, 2):                                       # the second call adds into the same buffers: exactly twice
        L.call("nerf_wgrad", dz, ldz, zc0, n_out, hin, ldh, hc0, n_in, dw, ldw, wc0, db if bias else None, P)
        torch.cuda.synchronize()
        got = dw.view(n_out, ldw)
        block = got[:, wc0:wc0 + n_in]
        bad = (block.double() != call * want_w)
        assert not bool(bad.any()), (f"P={P} scale={scale:g} call {call}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                                     f"{bad.nonzero()[0].tolist()}: got {block[bad][0].item()!r}, want {(call * want_w)[bad][0].item()!r}")
        assert bool((got[:, :wc0] == 0).all() and (got[:, wc0 + n_in:] == 0).all()), f"P={P}: columns outside the block were written"
        assert _intact(whole_w, n_out * ldw) and _intact(whole_b, n_out), f"P={P}: a sentinel around dw / db was overwritten"
        if bias:
            assert torch.equal(db.double(), call * want_b), f"P={P} scale={scale:g} call {call}: db differs"
        else:
            assert bool((db == 0).all())
        _probes["calls_bit_equal"] += 1


@pytest.mark.parametrize("name", list(R.probe_layouts()))
def test_integer_probe_is_bit_equal(amd, cus, name):
    layout = R.probe_layouts()[name]
    (ldz, zc0, n_out), (ldh, hc0, n_in), _, _ = layout
    forms = set()
    for P, form in R.probe_counts(layout, cus):
        row, got = R.wgrad_form(n_out, n_in, ldz, zc0, ldh, hc0, P, cus)          # (torch allocations are 512-byte aligned)
        assert got == form, (name, P, got, form)                                 # no silent fallback: the case runs the form it is listed under
        forms.add((row, form))
        assert R.PROBE_MAX ** 2 * P * 2 < 2 ** 24
        for scale in (1.0, 2.0 ** -20):
            _probe(amd, layout, P, scale, seed=P + n_out)
    print(f"{name}: (table row, form) visited: {sorted(forms, key=str)}")


# ================================================================================ 3: nerf_mlp_backward from the kernel's own operands
def _rays(P, seed):
    """P one-sample rays: the chain kernels are not under test, only their rows are needed."""
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.0, 0.0, 4.0]).expand(P, 3).contiguous().cuda()
    d = torch.randn(P, 3, generator=gen) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
    d = (d / d.norm(dim=-1, keepdim=True)).contiguous().cuda()
    t = (torch.rand(P, 1, generator=gen) * 4 + 2).cuda().contiguous()
    return o, d, t


def _gradient(P, seed, density_only, rows=None):
    """d loss / d raw [pad32(P), 4]: random normal times 1e-3 on `rows` (all of them when None), zero elsewhere, NaN behind row P - 1."""
    gen = torch.Generator().manual_seed(seed)
    G = torch.randn(P, 4, generator=gen) * 1e-3
    if rows is not None:
        keep = torch.zeros(P, dtype=torch.bool)
        keep[torch.as_tensor(rows, dtype=torch.long)] = True
        G[~keep] = 0.0
    if density_only:
        G[:, :3] = 0.0
    full = torch.full((R.pad32(P), 4), float("nan"))
    full[:P] = G
    return full.cuda().contiguous()


class Run:
    """One forward + backward through the C ABI; keeps every buffer the weight-gradient kernels read and wrote."""

    def __init__(self, amd, net, precision, density_only, P, G, seed, masked_valid=None, save_fill=float("nan")):
        L = amd._lib
        self.P, self.precision, self.dens = P, precision, density_only
        net.precision = precision
        prec = L.PRECISIONS[precision]
        o, d, t = _rays(P, seed)
        self.params = [p.detach().contiguous() for p in net.model.ordered_params()]
        assert [tuple(p.shape) for p in self.params] == R.PARAM_SHAPES
        pk, pk_b = net.packed(""), net.packed_bwd("")
        raw = torch.empty(P, 1, 4, device="cuda")
        self.save = torch.full((int(L.call("nerf_train_save_floats", P)),), save_fill, device="cuda")
        self.gsave = torch.full((int(L.call("nerf_train_grad_floats", P)),), float("nan"), device="cuda")    # a read of a row nobody wrote shows
        g_t = torch.empty(P, 1, device="cuda")
        self.grads = [torch.zeros_like(p) for p in self.params]
        rays = (o, d, t, 1, P, 1)
        self.draw = G.view(-1)
        if masked_valid is None:
            fwd = "nerf_mlp_forward_rays_save_density" if density_only else "nerf_mlp_forward_rays_save"
            bwd = "nerf_mlp_backward_density" if density_only else "nerf_mlp_backward"
            L.call(fwd, *rays, pk, raw, self.save, prec)
            L.call(bwd, *rays, pk_b, G, self.save, self.gsave, g_t, self.grads, prec)
        else:
            index = torch.full((P,), -7, dtype=torch.int32, device="cuda")
            count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            ws_c = torch.empty(int(L.call("nerf_compact_valid_workspace_bytes", P)), dtype=torch.uint8, device="cuda")
            L.call("nerf_compact_valid", masked_valid, P, index, count, ws_c)
            ws = torch.zeros(int(L.call("nerf_mlp_backward_masked_workspace_bytes", P)), dtype=torch.uint8, device="cuda")
            L.call("nerf_mlp_forward_rays_save_masked", *rays, index, count, pk, raw, self.save, prec)
            L.call("nerf_mlp_backward_masked", *rays, index, count, pk_b, G, self.save, self.gsave, g_t, self.grads, prec, ws)
            self.draw = ws[:P * 16].view(torch.float32)       # the compact incoming gradient: the first piece of the workspace
            self.count = int(count.item())
        torch.cuda.synchronize()
        net.precision = "f32"

    def live_list(self):
        """(flags, live list, count) as the backward left them behind the rows of gsave."""
        P, gi = self.P, self.gsave.view(torch.int32)
        n = int(gi[R.Grad.off_count(P)].item())
        return (gi[R.Grad.off_flags(P):R.Grad.off_flags(P) + R.Grad.n_tiles(P)].tolist(),
                gi[R.Grad.off_live(P):R.Grad.off_live(P) + max(n, 0)].tolist(), n)

    def check(self, rows, big_family, small_form, tag):
        """Every job from its own operands, over `rows` (the point rows its kernel integrates); every element, no exemption."""
        P, bufs = self.P, {"draw": self.draw, "save": self.save, "gsave": self.gsave}
        rows = torch.as_tensor(list(rows), dtype=torch.long, device=self.save.device)
        failures, touched = [], set()
        for job in R.jobs(self.dens):
            dz, hin = job.operands(bufs, P)
            dz, hin = dz[rows], hin[rows]
            assert bool(torch.isfinite(dz).all() and torch.isfinite(hin).all()), f"{tag} {job.name}: an operand row the kernel reads was never written"
            bf16 = job.big and self.precision == "f32x"
            family = (big_family if job.big else "small_" + small_form)
            truth, bound = R.truth_and_bound(dz, hin, **(R.BF16X3_DW if bf16 else R.F32_DW))
            idx, _, wc0 = job.w
            got = self.grads[idx][:, wc0:wc0 + job.n_in].double()
            err = (got - truth).abs()
            ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
            ratio = torch.nan_to_num(ratio, nan=float("inf"))
            worst = float(ratio.max())
            _note(f"{family}/dW", worst)
            touched.add(idx)
            if worst > 1.0:
                o, i = divmod(int(ratio.argmax()), job.n_in)
                failures.append(f"{job.name} dW: {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound, worst err / bound "
                                f"{worst:.3g} at [{o}, {i}]: got {got[o, i].item():.9g}, truth {truth[o, i].item():.9g}, bound {bound[o, i].item():.3g}")
            if job.b is not None:
                tb, bb = R.colsum_and_bound(dz)
                gb = self.grads[job.b].double()
                eb = (gb - tb).abs()
                rb = torch.where(bb > 0, eb / bb, torch.where(eb > 0, torch.full_like(eb, float("inf")), torch.zeros_like(eb)))
                rb = torch.nan_to_num(rb, nan=float("inf"))
                _note(f"{family}/db", float(rb.max()))
                touched.add(job.b)
                if float(rb.max()) > 1.0:
                    o = int(rb.argmax())
                    failures.append(f"{job.name} db: {int((rb > 1).sum())} of {rb.numel()} over the bound, worst {float(rb.max()):.3g} at [{o}]: "
                                    f"got {gb[o].item():.9g}, truth {tb[o].item():.9g}, bound {bb[o].item():.3g}")
        for i, g in enumerate(self.grads):                    # what no job feeds (density only: the colour branch) stays exactly zero
            if i not in touched and not bool((g == 0).all()):
                failures.append(f"gradient {i} has no job in this entry and is not zero")
        assert not failures, f"{tag}: " + "; ".join(failures)

    def assert_unmarked_rows_are_zero(self, marked, tag):
        """dense form: the chain wrote +-0 into every gsave row of a point without incoming gradient"""
        P = self.P
        keep = torch.ones(P, dtype=torch.bool, device=self.gsave.device)
        keep[torch.as_tensor(list(marked), dtype=torch.long, device=self.gsave.device)] = False
        regions = [(R.Grad.off_gz(P, l), 256) for l in range(8)]
        if not self.dens:
            regions += [(R.Grad.off_gzv(P), 128), (R.Grad.off_gf(P), 256)]
        for off, ld in regions:
            rows = self.gsave[off:off + R.pad32(P) * ld].view(R.pad32(P), ld)[:P][keep]
            assert bool((rows == 0).all()), f"{tag}: a gsave row of an unmarked point is not zero (region at {off})"


def _small_form(P, cus, live):
    """the form the six small-layer jobs run in (they are all ring rows: the table mirror says so for each)"""
    forms = set()
    for job in R.SMALL_JOBS:
        forms.add(R.wgrad_form(job.n_out, job.n_in, job.dz[2], job.dz[3], job.hin[2], job.hin[3], P, cus, live=live)[1])
    assert len(forms) == 1, forms
    return forms.pop()


_DENSE_CASES = [(prec, dens, regime) for prec in ("f32x", "f32") for dens in (False, True)
                for regime in R.backward_counts(prec, dens, 256)]


@pytest.mark.parametrize("kind", ["markers", "dense"])
@pytest.mark.parametrize("precision,density_only,regime", _DENSE_CASES)
def test_backward_dense_form(amd, net, cus, monkeypatch, precision, density_only, regime, kind):
    """Every row of every point is integrated (NERF_DEAD_TILE_SKIP=0 where the count is a multiple of 32)."""
    monkeypatch.setenv("NERF_DEAD_TILE_SKIP", "0")
    P = R.backward_counts(precision, density_only, cus)[regime]
    n_jobs = R.n_big_jobs(density_only)
    family, slices = R.big_job_slices(precision, P, n_jobs, cus)
    want_family = {"layer_by_layer_ring": "ring_single", "layer_by_layer_vec": "vec_plain"}.get(regime, "bf16x3" if precision == "f32x" else "ring_batched")
    assert family == want_family, (regime, P, family)                 # the case runs the kernel it is listed under
    small = _small_form(P, cus, live=False)
    assert small == (R.RING if P % 32 == 0 else R.PLAIN)
    tag = f"{precision}{'/density' if density_only else ''} {regime} P={P} [{family}]"
    if kind == "dense":
        run = Run(amd, net, precision, density_only, P, _gradient(P, P, density_only), seed=P)
        assert run.live_list()[2] == -1                               # no list was built
        run.check(range(P), family, small, tag + " dense")
        return
    classes = R.marker_classes(P, slices)
    for k, rows in enumerate(R.marker_sets(classes)):
        assert 1 <= len(rows) <= 8
        run = Run(amd, net, precision, density_only, P, _gradient(P, P + k, density_only, rows), seed=P)
        run.assert_unmarked_rows_are_zero(rows, tag)
        run.check(range(P), family, small, f"{tag} markers {rows}")


_LIST_CASES = [(n_live, kind) for n_live in R.LIST_LIVE for kind in (("markers", "dense") if n_live in (1, 2) else ("dense",))]


@pytest.mark.parametrize("n_live,kind", _LIST_CASES)
@pytest.mark.parametrize("density_only", [False, True])
@pytest.mark.parametrize("precision", ["f32x", "f32"])
def test_backward_list_form(amd, net, cus, monkeypatch, precision, density_only, n_live, kind):
    """Dead-tile skipping on (the default): whole tiles of the incoming gradient are zero, the kernels walk the live-tile list.  The
    truth sums the rows of live tiles only; gsave is NaN wherever the chain did not write, so a read of a dead row shows."""
    monkeypatch.delenv("NERF_DEAD_TILE_SKIP", raising=False)
    P, n_jobs = R.LIST_P, R.n_big_jobs(density_only)
    tiles = R.live_tiles_of(n_live)
    family, slices = R.big_job_slices(precision, P, n_jobs, cus, n_live)
    assert family == ("bf16x3" if precision == "f32x" else "ring_batched")
    assert _small_form(P, cus, live=True) == R.LIST
    tag = f"{precision}{'/density' if density_only else ''} list P={P} n_live={n_live}"
    if kind == "dense":
        row_sets = [[r for t in tiles for r in range(32 * t, 32 * t + 32)]]
    else:
        classes = R.marker_classes(P, slices, tiles)
        assert set(R.LIST_CLASSES) <= set(classes)
        row_sets = R.marker_sets(classes)
    for k, rows in enumerate(row_sets):
        G = _gradient(P, P + n_live + k, density_only, rows)
        nz = (G[:P, 3] != 0) if density_only else (G[:P] != 0).any(1)
        live = nz.view(-1, 32).any(1).nonzero().flatten().tolist()                # the live set, computed from G itself
        assert kind == "markers" or live == tiles
        run = Run(amd, net, precision, density_only, P, G, seed=P)
        flags, lst, count = run.live_list()
        assert count == len(live) and lst == live and [i for i, f in enumerate(flags) if f] == live, (tag, count, lst[:8], live[:8])
        run.check([r for t in live for r in range(32 * t, 32 * t + 32)], family + "_list", "list", f"{tag} {kind} set {k}")


@pytest.mark.parametrize("precision", ["f32x", "f32"])
def test_backward_masked_on_a_random_half(amd, net, cus, monkeypatch, precision):
    """nerf_mlp_backward_masked with NERF_DEAD_TILE_SKIP=0: the compact rows 0 .. M - 1 of a random half of the ids, M % 32 != 0; the
    live tiles are the occupied ones, the rows behind M - 1 in the last of them carry a zero gradient."""
    monkeypatch.setenv("NERF_DEAD_TILE_SKIP", "0")
    P = R.LIST_P
    valid = (torch.rand(P, generator=torch.Generator().manual_seed(11)) < 0.5).to(torch.uint8)
    if int(valid.sum()) % 32 == 0:
        valid[int((valid == 0).nonzero()[0])] = 1
    M = int(valid.sum())
    assert M % 32 != 0 and 0 < M < P
    run = Run(amd, net, precision, False, P, _gradient(P, 12, False), seed=P, masked_valid=valid.cuda(), save_fill=12345.0)
    assert run.count == M
    occupied = (M + 31) // 32
    flags, lst, count = run.live_list()
    assert count == occupied and lst == list(range(occupied))
    compact = run.draw[:P * 4].view(P, 4)
    assert bool((compact[M:] == 0).all()) and bool((compact[:M] != 0).any())
    family, _ = R.big_job_slices(precision, P, 8, cus, occupied)
    run.check(range(32 * occupied), family + "_list", "list", f"{precision} masked M={M}")
