"""CPU checks of tests/wgrad_reference.py, the yardstick of tests/test_gpu_wgrad_exact.py: the bf16 split is exact and its dropped
products are as small as the GPU bound says, the table mirror chooses what csrc/nerf_wgrad_table.h chooses, the work partitions tile
their ranges, the chosen point counts visit every slice / ring regime, and the integer probes are exact by construction."""
import os

import pytest
import torch

import wgrad_reference as R
from conftest import GOLDEN

CUS = (256, 304, 64, 8, 1)


def _random_fp32(n, seed):
    """n fp32 values with uniform significands, both signs, exponents across 2^-60 .. 2^60."""
    gen = torch.Generator().manual_seed(seed)
    m = 1.0 + torch.rand(n, generator=gen, dtype=torch.float64)
    e = torch.randint(-60, 61, (n,), generator=gen).double()
    s = torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1
    return (s * m * 2.0 ** e).float()


def _all_bits_set():
    """values whose 24 significand bits are all ones, across the same binades, and their neighbours"""
    top = torch.tensor([2.0 - 2.0 ** -23, 2.0 - 2.0 ** -22, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, 1.0 + 2.0 ** -7 + 2.0 ** -15,
                        1.0 + 2.0 ** -7 - 2.0 ** -23],            # the last: hi = 1, mid and lo all ones, the largest residuals there are
                       dtype=torch.float64)
    e = torch.arange(-60, 61).double()
    v = (top[:, None] * 2.0 ** e[None, :]).reshape(-1)
    return torch.cat([v, -v]).float()


def test_split_is_exact():
    x = torch.cat([_random_fp32(100000, 1), _all_bits_set()])
    hi, mid, lo = R.split3_bf16(x)
    for part in (hi, mid, lo):
        assert torch.all((part.view(torch.int32) & 0xffff) == 0)                # each part is a bf16 value
    assert torch.equal(((hi + mid) + lo).view(torch.int32), x.view(torch.int32))   # exact in fp32, in the kernel's own order
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    # what the dropped-product figure follows from
    assert torch.all((x - hi).abs().double() < 2.0 ** -7 * x.abs().double())
    r1 = (x - hi).double()
    assert torch.all((r1 - mid.double()).abs() <= 2.0 ** -7 * r1.abs())
    assert torch.all(mid.abs().double() < 2.0 ** -7 * x.abs().double()) and torch.all(lo.abs().double() < 2.0 ** -14 * x.abs().double())


def test_dropped_products_are_below_the_figure_of_the_gpu_bound():
    a, b = _random_fp32(100000, 2), _random_fp32(100000, 3)
    typical = R.dropped_products(a, b)
    worst_in = _all_bits_set()
    worst = R.dropped_products(worst_in[:, None].expand(-1, worst_in.numel()).reshape(-1),
                               worst_in[None, :].expand(worst_in.numel(), -1).reshape(-1))
    print(f"dropped products / |a b|: random operands median 2^{torch.log2(typical.median()).item():.2f}, max 2^{torch.log2(typical.max()).item():.2f}; "
          f"all-ones significands max 2^{torch.log2(worst.max()).item():.3f}")
    assert typical.max() < R.DROPPED_PRODUCT_BOUND and worst.max() < R.DROPPED_PRODUCT_BOUND
    # "below 2^-24" is the typical size only: the worst case (significand 1.0000000 followed by sixteen ones) is eight times that,
    # half of the bound
    assert worst.max() > 2.0 ** -21.1 and typical.max() > 2.0 ** -24 and typical.median() < 2.0 ** -24
    assert R.BF16X3_DROPPED == 17 and R.DROPPED_PRODUCT_BOUND / R.U < R.BF16X3_DROPPED


def test_table_mirror_chooses_what_the_header_chooses():
    """against tests/golden/wgrad_choice.txt, the record tests/test_wgrad_choice.py holds the header itself to"""
    name = {R.GENERIC: "f32", R.VEC: "vec", R.VEC_RING: "vec"}
    n = 0
    for line in open(os.path.join(GOLDEN, "wgrad_choice.txt")).read().splitlines():
        n_out, n_in, facts, inst, osplit, isplit = line.split()
        n_out, n_in, facts = int(n_out), int(n_in), int(facts)
        row, form = R.wg_choose(n_out, n_in, bool(facts & 1), bool(facts & 2), bool(facts & 4), bool(facts & 8))
        if form == R.NO_LIST_KERNEL:
            got = ("none", 0, 0)
        else:
            kind, wo, wi, os_, is_ = R.WG_ROWS[row][:5]
            got = (f"{name[kind]}<{wo},{wi}>" if form == R.PLAIN else f"{form}<{wo},{wi},16>", os_, is_)
        assert got == (inst.replace("w256", "vec<4,4>"), int(osplit), int(isplit)), line
        n += 1
    assert n == 22 * 22 * 16


def test_job_list_covers_every_gradient_once():
    for dens in (False, True):
        jobs = R.jobs(dens)
        assert len(jobs) == (10 if dens else 14) and R.n_big_jobs(dens) == (7 if dens else 8)
        cover = [torch.zeros(s, dtype=torch.int32) for s in R.PARAM_SHAPES]
        for j in jobs:
            idx, ldw, wc0 = j.w
            assert R.PARAM_SHAPES[idx] == (j.n_out, ldw)
            cover[idx][:, wc0:wc0 + j.n_in] += 1
            if j.b is not None:
                assert R.PARAM_SHAPES[j.b] == (j.n_out,)
                cover[j.b] += 1
            assert not j.big or (j.n_out, j.n_in, j.dz[2], j.dz[3], j.hin[2], j.hin[3]) == (256, 256, 256, 0, 256, 0)
        colour = {R.P_WV, R.P_BV, R.P_WF, R.P_BF, R.P_WR, R.P_BR}
        for i, c in enumerate(cover):
            assert torch.all(c == (0 if dens and i in colour else 1)), i


def test_layout_regions_do_not_overlap():
    for P in (1, 31, 32, 33, 185, 2048, 2592):
        rows = R.pad32(P)
        ends = [R.Save.off_pe(P) + rows * 64, R.Save.off_dpe(P) + rows * 32] + [R.Save.off_h(P, l) + rows * 256 for l in range(8)] + \
               [R.Save.off_f(P) + rows * 256, R.Save.off_hv(P) + rows * 128]
        starts = [R.Save.off_pe(P), R.Save.off_dpe(P)] + [R.Save.off_h(P, l) for l in range(8)] + [R.Save.off_f(P), R.Save.off_hv(P), R.Save.off_bits(P)]
        assert starts[1:] == ends and R.Save.floats(P) == R.Save.off_stamp(P) + 4
        g_starts = [R.Grad.off_gzv(P), R.Grad.off_gf(P)] + [R.Grad.off_gz(P, l) for l in range(7, -1, -1)] + [R.Grad.off_flags(P)]
        g_ends = [rows * 128, R.Grad.off_gf(P) + rows * 256] + [R.Grad.off_gz(P, l) + rows * 256 for l in range(7, -1, -1)]
        assert g_starts[1:] == g_ends
        assert R.Grad.off_flags(P) + R.Grad.n_tiles(P) <= R.Grad.off_live(P) and R.Grad.off_live(P) + R.Grad.n_tiles(P) <= R.Grad.off_count(P)


def _all_backward_cases(C):
    for precision in ("f32", "f32x"):
        for dens in (False, True):
            for regime, P in R.backward_counts(precision, dens, C).items():
                yield precision, dens, regime, P


@pytest.mark.parametrize("C", CUS)
def test_partitions_are_sound(C):
    for precision, dens, _, P in _all_backward_cases(C):
        n_jobs = R.n_big_jobs(dens)
        assert R.tiles_without_gap(R.bf16x3_slices(P, n_jobs, C), (P + 15) // 16), (P, n_jobs)
        if P % 16 == 0:
            assert R.tiles_without_gap(R.batched_ring_slices(P, n_jobs, C), P // 16, empties_last=False)
            if R.ring256_single_ok(P, C):
                assert R.tiles_without_gap(R.single_ring_slices(P, C), P // 16, empties_last=False)
    for n_live in R.LIST_LIVE:
        for n_jobs in (7, 8):
            assert R.tiles_without_gap(R.bf16x3_slices(R.LIST_P, n_jobs, C, n_live), 2 * n_live)
            assert R.tiles_without_gap(R.batched_ring_slices(R.LIST_P, n_jobs, C, n_live), 2 * n_live, empties_last=False)
        assert R.tiles_without_gap(R.small_ring_slices(R.LIST_P, C, n_live), n_live, empties_last=False)
    for P in R.ring_counts(C):
        assert R.tiles_without_gap(R.small_ring_slices(P, C), P // 32, empties_last=False)
        assert all(b > a for a, b in R.small_ring_slices(P, C))                 # host contract 2: no workgroup without a group
    for P in R.ring256_counts(C):
        assert R.ring256_single_ok(P, C) and P < 16417
        sl = R.single_ring_slices(P, C)
        assert R.tiles_without_gap(sl, P // 16, empties_last=False) and all(b > a for a, b in sl)
    # the fp32 ring's ranges are floors of a product: in order and complete by construction, but empty ones may stand anywhere
    assert R.ring_slices(3, 8) == [(0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 2), (2, 2), (2, 3)]
    assert not R.tiles_without_gap([(0, 2), (3, 4)], 4) and not R.tiles_without_gap([(0, 0), (0, 4)], 4)


def test_every_required_regime_is_present():
    R.check_coverage(256)


def test_integer_probes_are_exact_by_construction():
    for C in CUS:
        for layout in R.probe_layouts().values():
            for P, _ in R.probe_counts(layout, C):
                assert R.PROBE_MAX ** 2 * P < 2 ** 24 and 2 * R.PROBE_MAX ** 2 * P < 2 ** 24          # one call, and the second into the same buffers
    # float64 carries the integer product exactly: the GPU test forms it there
    gen = torch.Generator().manual_seed(5)
    dz = torch.randint(-8, 9, (16385, 7), generator=gen)
    hin = torch.randint(-8, 9, (16385, 5), generator=gen)
    truth, bound = R.truth_and_bound(dz.float(), hin.float(), **R.F32_DW)
    assert torch.equal(truth.long(), dz.T @ hin) and torch.equal(truth, truth.float().double())
    assert torch.equal(R.colsum_and_bound(dz.float())[0].long(), dz.sum(0))
    assert torch.equal((truth * 2.0 ** -20).float().double(), truth * 2.0 ** -20)


def test_truth_and_bound_count_non_zero_terms_only():
    dz = torch.tensor([[1.0, 0.0], [2.0, 3.0], [0.0, 0.0]])
    hin = torch.tensor([[4.0], [0.5], [7.0]])
    truth, bound = R.truth_and_bound(dz, hin, extra=2)
    assert truth.tolist() == [[5.0], [1.5]] and bound.tolist() == [[(2 + 2) * R.U * 5.0], [(1 + 2) * R.U * 1.5]]
    _, bound6 = R.truth_and_bound(dz, hin, **R.BF16X3_DW)
    assert bound6.tolist() == [[(12 + 19) * R.U * 5.0], [(6 + 19) * R.U * 1.5]]
    s, b = R.colsum_and_bound(dz)
    assert s.tolist() == [3.0, 3.0] and b.tolist() == [3 * R.U * 3.0, 2 * R.U * 3.0]
