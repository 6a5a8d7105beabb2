"""What tests/test_gpu_wgrad_exact.py holds the weight-gradient kernels to (csrc/nerf_wgrad_f32.hip.inc, nerf_wgrad_bf16x3.hip.inc,
nerf_wgrad_table.h), written in plain torch from the formulas and the host code, importing nothing of the package:

    dW[o][i] += sum_p dZ[p][o] Hin[p][i]        db[o] += sum_p dZ[p][o]

  layout mirror     where the rows of a training step live: TrainSave (pe, dpe, h0..h7, f, hv) and TrainGrad (gzv, gf, gz(l), flags,
                    live, count) as functions of the point count P
  job list          the 14 GEMMs mlp_backward_impl launches (six small-layer jobs, eight 256 x 256 jobs; three and seven for density only): which
                    region is dZ, which is Hin, pitches, column offsets, and the gradient block and bias each one feeds
  table mirror      nerf::kWgRows / wg_choose and the conditions wgrad_impl and mlp_backward_impl put in front of them
  work partitions   which steps / groups each workgroup slice of the 256 x 256 kernels integrates.  They only choose inputs and let a
                    test assert that it visits a regime; they never decide what a correct result is
  truth and bound   float64 sums over the kernel's own fp32 operands and the sums of absolute terms that rounding bounds scale with
  bf16 split        split3_bf16 of the bf16x3 kernel in float32: truncate to the upper 16 bits, subtract, twice

Bounds (u = 2^-24; n = rows with a non-zero term in that element, sums over those rows; they hold for any summation order):
  fp32 kernels      |dW - truth| <= (n + 2) u sum|term|,  |db - truth| <= (n + 1) u sum|dz|
  bf16x3            |dW - truth| <= (6 n + 2 + 17) u sum|term|: the six kept products of a term are exact in fp32 and enter the fp32
                    accumulator one by one (6 n roundings at most, each assumed to be to nearest); the three dropped ones are below
                    (2^-20 + 2^-27) |term| < 16.2 u |term| (dropped_product_bound), hence 17.  db is summed in fp32 from unsplit values.
"""
import json
import os
import shutil

import torch

U = 2.0 ** -24
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_JSON = os.path.join(REPO, "profiles", "wgrad_bounds.json")

# ------------------------------------------------------------------------------------------------ layout mirror (floats)


def pad32(P):
    return (P + 31) & ~31


class Save:
    """TrainSave of csrc/nerf_mlp_common.h: every region holds pad32(P) rows."""
    @staticmethod
    def off_pe(P): return 0
    @staticmethod
    def off_dpe(P): return pad32(P) * 64
    @staticmethod
    def off_h(P, l): return pad32(P) * (96 + 256 * l)
    @staticmethod
    def off_f(P): return pad32(P) * (96 + 2048)
    @staticmethod
    def off_hv(P): return pad32(P) * (96 + 2304)
    @staticmethod
    def off_bits(P): return pad32(P) * (96 + 2304 + 128)
    @staticmethod
    def off_stamp(P): return Save.off_bits(P) + (pad32(P) // 32) * 9 * 256
    @staticmethod
    def floats(P): return Save.off_stamp(P) + 4


class Grad:
    """TrainGrad of csrc/nerf_mlp_common.h: the rows, then int32 flags, live list and count."""
    @staticmethod
    def off_gzv(P): return 0
    @staticmethod
    def off_gf(P): return pad32(P) * 128
    @staticmethod
    def off_gz(P, l): return pad32(P) * (384 + 256 * (7 - l))
    @staticmethod
    def n_tiles(P): return pad32(P) // 32
    @staticmethod
    def off_flags(P): return pad32(P) * (384 + 2048)
    @staticmethod
    def off_live(P): return Grad.off_flags(P) + ((Grad.n_tiles(P) + 3) & ~3)
    @staticmethod
    def off_count(P): return Grad.off_live(P) + ((Grad.n_tiles(P) + 3) & ~3)
    @staticmethod
    def floats(P): return Grad.off_count(P) + 4


# ------------------------------------------------------------------------------------------------ job list
# Parameter order of one sub-model (state_dict order): pts_linears.l -> 2l, 2l + 1; views 16, 17; feature 18, 19; alpha 20, 21; rgb 22, 23
P_WV, P_BV, P_WF, P_BF, P_WA, P_BA, P_WR, P_BR = 16, 17, 18, 19, 20, 21, 22, 23


class Job:
    """One GEMM of mlp_backward_impl.  dz / hin: (buffer, region offset as a function of P, pitch, first column, width), buffer one of
    "draw", "save", "gsave".  w: (parameter index, pitch, first column).  b: parameter index or None.  colour: skipped by the
    density-only entry.  big: one of the 256 x 256 jobs of the batched launch."""

    def __init__(self, name, dz, hin, w, b, colour, big):
        self.name, self.dz, self.hin, self.w, self.b, self.colour, self.big = name, dz, hin, w, b, colour, big

    @staticmethod
    def _view(spec, bufs, P):
        buf, off, ld, c0, n = spec
        base = off(P)
        return bufs[buf][base:base + pad32(P) * ld].view(pad32(P), ld)[:, c0:c0 + n]

    def operands(self, bufs, P):
        """-> (dz [pad32(P), n_out], hin [pad32(P), n_in]) as views of the flat fp32 buffers {"draw", "save", "gsave"} ("draw" must
        be given padded to pad32(P) rows)."""
        return self._view(self.dz, bufs, P), self._view(self.hin, bufs, P)

    @property
    def n_out(self): return self.dz[4]
    @property
    def n_in(self): return self.hin[4]


def _gz(l): return lambda P: Grad.off_gz(P, l)
def _h(l): return lambda P: Save.off_h(P, l)


_DRAW = lambda P: 0
# the WG(...) lines of mlp_backward_impl, in launch order
SMALL_JOBS = [
    Job("rgb_linear", ("draw", _DRAW, 4, 0, 3), ("save", Save.off_hv, 128, 0, 128), (P_WR, 128, 0), P_BR, True, False),
    Job("alpha_linear", ("draw", _DRAW, 4, 3, 1), ("save", _h(7), 256, 0, 256), (P_WA, 256, 0), P_BA, False, False),
    Job("views_feature", ("gsave", Grad.off_gzv, 128, 0, 128), ("save", Save.off_f, 256, 0, 256), (P_WV, 283, 0), P_BV, True, False),
    Job("views_dirs", ("gsave", Grad.off_gzv, 128, 0, 128), ("save", Save.off_dpe, 32, 0, 27), (P_WV, 283, 256), None, True, False),
    Job("pe_skip", ("gsave", _gz(5), 256, 0, 256), ("save", Save.off_pe, 64, 0, 63), (10, 319, 0), 11, False, False),
    Job("pe_layer0", ("gsave", _gz(0), 256, 0, 256), ("save", Save.off_pe, 64, 0, 63), (0, 63, 0), 1, False, False),
]
# its job[] array: feature_linear, then layers 7..1 with the skip layer's hidden part
BIG_JOBS = [Job("feature_linear", ("gsave", Grad.off_gf, 256, 0, 256), ("save", _h(7), 256, 0, 256), (P_WF, 256, 0), P_BF, True, True)]
for _l in range(7, 0, -1):
    if _l == 5:
        BIG_JOBS.append(Job("layer5_hidden", ("gsave", _gz(5), 256, 0, 256), ("save", _h(4), 256, 0, 256), (10, 319, 63), None, False, True))
    else:
        BIG_JOBS.append(Job(f"layer{_l}", ("gsave", _gz(_l), 256, 0, 256), ("save", _h(_l - 1), 256, 0, 256), (2 * _l, 256, 0), 2 * _l + 1,
                            False, True))


def jobs(density_only):
    return [j for j in SMALL_JOBS + BIG_JOBS if not (density_only and j.colour)]


def n_big_jobs(density_only):
    return sum(1 for j in jobs(density_only) if j.big)


PARAM_SHAPES = [s for l in range(8) for s in ((256, 63 if l == 0 else 319 if l == 5 else 256), (256,))] + \
               [(128, 283), (128,), (256, 256), (256,), (1, 256), (1,), (3, 128), (3,)]

# ------------------------------------------------------------------------------------------------ table mirror
GENERIC, VEC, VEC_RING = "generic", "vec", "vec_ring"
ANY, HIN8, ALIGNED16 = "any", "hin8", "aligned16"
PLAIN, RING, LIST, NO_LIST_KERNEL, RING256 = "plain", "ring", "list", "no-list-kernel", "ring256"
#          kind      wo wi os is align      exact_out exact_in
WG_ROWS = [(VEC, 4, 4, 2, 2, ALIGNED16, True, True),
           (VEC_RING, 4, 1, 2, 2, ALIGNED16, True, False),
           (VEC_RING, 4, 2, 1, 4, ALIGNED16, True, True),
           (VEC_RING, 1, 1, 4, 1, ANY, True, False),
           (VEC_RING, 1, 2, 1, 4, HIN8, False, True),
           (VEC_RING, 1, 1, 1, 4, ANY, False, False),
           (GENERIC, 1, 2, 1, 4, ANY, False, False),
           (GENERIC, 1, 1, 4, 1, ANY, False, False),
           (GENERIC, 1, 1, 2, 2, ANY, False, False),
           (GENERIC, 1, 2, 2, 2, ANY, False, False),
           (GENERIC, 2, 2, 2, 2, ANY, False, False),
           (GENERIC, 2, 4, 2, 2, ANY, False, False),
           (GENERIC, 4, 1, 2, 2, ANY, False, False),
           (GENERIC, 4, 4, 2, 2, ANY, False, False)]


def wg_choose(n_out, n_in, aligned, hin8, ring, live):
    """nerf::wg_choose -> (row index, form): the first row that covers the shape and whose alignment the operands have."""
    for i, (kind, wo, wi, osplit, isplit, align, exact_out, exact_in) in enumerate(WG_ROWS):
        outs, ins = 32 * wo * osplit, 32 * wi * isplit
        if (n_out == outs if exact_out else n_out <= outs) and (n_in == ins if exact_in else n_in <= ins) and \
                (align == ANY or (align == HIN8 and hin8) or (align == ALIGNED16 and aligned)):
            r = kind == VEC_RING and ring
            return i, (LIST if r else NO_LIST_KERNEL) if live else (RING if r else PLAIN)
    return -1, NO_LIST_KERNEL


def plain_grid(P, num_cus):
    """wgrad_impl's grid of the plain forms: at least 256 point pairs per workgroup, at most one workgroup per CU."""
    return max(1, min(num_cus, ((P + 1) // 2 + 255) // 256))


def ring256_single_ok(P, num_cus):
    """wgrad_impl's test for one aligned 256 x 256 layer on the ring launch (both pitches are far below 2^28 floats here)."""
    return P % 16 == 0 and P // 16 >= plain_grid(P, num_cus)


def wgrad_form(n_out, n_in, ldz, zc0, ldh, hc0, P, num_cus, live=False, base_aligned=True):
    """What wgrad_impl launches for a call -> (row index or None, form); base_aligned: both operands start on 16 bytes."""
    aligned = ldz % 4 == 0 and ldh % 4 == 0 and zc0 % 4 == 0 and hc0 % 4 == 0 and base_aligned
    hin8 = ldh % 2 == 0 and hc0 % 2 == 0 and base_aligned
    if n_out == 256 and n_in == 256 and aligned and ring256_single_ok(P, num_cus):
        return None, RING256
    return wg_choose(n_out, n_in, aligned, hin8, P % 32 == 0, live)


def batched_ring_ok(P, num_cus):
    """mlp_backward_impl's test for the fp32 256 x 256 jobs in one ring launch; below it they go one by one through wgrad_impl."""
    return P % 16 == 0 and P // 16 >= num_cus // 8

# ------------------------------------------------------------------------------------------------ work partitions


def bf16x3_slices(P, n_jobs, num_cus, n_live=None):
    """nerf_wgrad256_bf16x3_kernel: the 16-point step range [s0, s1) of every slice of one job, empty ones included.  The host sizes
    the grid from the dense step count; with a live-tile list the steps are the halves of the live tiles."""
    dense_steps = (P + 15) // 16
    n_slices = max(1, min(num_cus // n_jobs, dense_steps))
    n_steps = dense_steps if n_live is None else 2 * n_live
    per = (n_steps + n_slices - 1) // n_slices
    return [(min(s * per, n_steps), min(s * per + per, n_steps)) for s in range(n_slices)]


def ring_slices(n_groups, n_slices):
    """wg_ring_job: the group range [g0, g1) of every slice."""
    return [(n_groups * s // n_slices, n_groups * (s + 1) // n_slices) for s in range(n_slices)]


def batched_ring_slices(P, n_jobs, num_cus, n_live=None):
    """The fp32 256 x 256 jobs in one launch: groups of 8 k-steps = 16 points (with a list: the halves of the live tiles)."""
    return ring_slices(P // 16 if n_live is None else 2 * n_live, max(1, num_cus // n_jobs))


def single_ring_slices(P, num_cus):
    """One 256 x 256 layer through wgrad_impl on the ring launch: one slice per workgroup of the plain grid."""
    return ring_slices(P // 16, plain_grid(P, num_cus))


def small_ring_slices(P, num_cus, n_live=None):
    """The small-layer ring kernels: groups of 16 k-steps = 32 points, one workgroup per group up to one per CU (list: one per CU)."""
    if n_live is not None:
        return ring_slices(n_live, num_cus)
    return ring_slices(P // 32, min(P // 32, num_cus))


def big_job_slices(precision, P, n_jobs, num_cus, n_live=None):
    """The 16-point unit ranges of the workgroups that integrate ONE 256 x 256 job inside nerf_mlp_backward, and the kernel family:
    "bf16x3", "ring_batched", "ring_single" (layer by layer, on the ring) or "vec_plain" (layer by layer, the <4,4> vector-load kernel,
    which splits 2-point pairs: returned in 16-point units rounded outwards, for marker placement only)."""
    if precision == "f32x":
        return "bf16x3", bf16x3_slices(P, n_jobs, num_cus, n_live)
    if batched_ring_ok(P, num_cus):
        return "ring_batched", batched_ring_slices(P, n_jobs, num_cus, n_live)
    assert n_live is None or ring256_single_ok(P, num_cus)
    if ring256_single_ok(P, num_cus):
        return "ring_single", ring_slices(P // 16 if n_live is None else 2 * n_live, plain_grid(P, num_cus))
    return "vec_plain", [(0, (P + 15) // 16)]


def tiles_without_gap(slices, n, empties_last=True):
    """True when the ranges tile [0, n) in order without gap or overlap and (empties_last) no empty range stands before a non-empty
    one.  The bf16x3 ranges are multiples of `per`, so their empty ones come last; the fp32 ring's are floors of a product and an
    empty one may stand anywhere (its workgroup exits before its first load)."""
    pos, seen_empty = 0, False
    for a, b in slices:
        if a >= b:
            seen_empty = True
            continue
        if (seen_empty and empties_last) or a != pos:
            return False
        pos = b
    return pos == n


# ------------------------------------------------------------------------------------------------ cases of the GPU tests
# every row of the table at the smallest shape that selects it: tests/test_gpu_training.py's _WGRAD_ROW_SHAPES and the 256 x 256 rows
WGRAD_ROW_SHAPES = [(256, 64), (128, 256), (128, 27), (1, 256), (3, 128), (33, 27), (33, 33), (64, 64), (64, 128), (65, 97), (128, 128)]
PROBE_SHAPES = WGRAD_ROW_SHAPES + [(256, 256)]
# (ldz, zc0, n_out), (ldh, hc0, n_in), (ldw, wc0), bias: tests/test_gpu_training.py's _SMALL_LAYOUTS
SMALL_LAYOUTS = {"rgb_linear": ((4, 0, 3), (128, 0, 128), (128, 0), True),
                 "alpha_linear": ((4, 3, 1), (256, 0, 256), (256, 0), True),
                 "views_feature": ((128, 0, 128), (256, 0, 256), (283, 0), True),
                 "views_dirs": ((128, 0, 128), (32, 0, 27), (283, 256), False),
                 "pe_skip": ((256, 0, 256), (64, 0, 63), (319, 0), True),
                 "pe_layer0": ((256, 0, 256), (64, 0, 63), (63, 0), True)}


def probe_layout(n_out, n_in, aligned):
    """test_wgrad_gemm's two layouts of a shape -> (ldz, zc0, n_out), (ldh, hc0, n_in), (ldw, wc0), bias."""
    ldz, zc0, ldh, hc0 = (n_out + 8, 4, n_in + 12, 8) if aligned else (n_out + 5, 2, n_in + 9, 4)
    return (ldz, zc0, n_out), (ldh, hc0, n_in), (n_in + 11, 7), True


def probe_layouts():
    """name -> layout, for the integer probes: every shape aligned and unaligned, then the six training layouts."""
    out = {}
    for n_out, n_in in PROBE_SHAPES:
        for aligned in (True, False):
            out[f"{n_out}x{n_in}-{'aligned' if aligned else 'unaligned'}"] = probe_layout(n_out, n_in, aligned)
    out.update(SMALL_LAYOUTS)
    return out


def plain_counts(num_cus):
    return [1, 2, 31, 33, 511, 513, min(512 * num_cus + 1, 16385)]


def ring_counts(num_cus):
    """one group per workgroup, the first workgroup with two, then uneven splits"""
    return sorted({32, 64, 32 * max(num_cus - 1, 1), 32 * num_cus, 32 * (num_cus + 1), 32 * (2 * num_cus + 1)})


def ring256_counts(num_cus):
    top = 512 * num_cus + 16
    if top >= 16417:
        top = max(p for p in range(16, 16417, 16) if ring256_single_ok(p, num_cus))
    return sorted({16, 32, 48, 512, 528, top})


def probe_counts(layout, num_cus):
    """[(P, expected form)] of one probe layout: the plain counts, and where the layout reaches a ring kernel those counts too."""
    (ldz, zc0, n_out), (ldh, hc0, n_in), _, _ = layout
    out = []
    for P in plain_counts(num_cus):
        out.append((P, PLAIN))
    row, form = wgrad_form(n_out, n_in, ldz, zc0, ldh, hc0, 32, num_cus)
    if form == RING:
        out += [(P, RING) for P in ring_counts(num_cus)]
    if (n_out, n_in) == (256, 256) and ldz % 4 == 0 and ldh % 4 == 0 and zc0 % 4 == 0 and hc0 % 4 == 0:
        out += [(P, RING256) for P in ring256_counts(num_cus)]
    return out


PROBE_MAX = 8                 # operands are integers in [-8, 8]: every term is at most 64 in magnitude


def backward_counts(precision, density_only, num_cus):
    """{regime: P} of the dense-form nerf_mlp_backward cases, derived from the device: S slices per 256 x 256 job."""
    S = max(1, num_cus // n_big_jobs(density_only))
    if precision == "f32x":
        def steps(per, ok):                  # the smallest step count that gives slices of `per` steps and passes `ok`
            return next((n for n in range((per - 1) * S + 1, per * S + 1) if ok(n)), per * S)
        return {"per1_short": 185, "per1_full": 16 * S,
                "per2_one_step_slice": 16 * steps(2, lambda n: n % 2 == 1),                 # ... and empty slices behind it
                "per2_ragged": 16 * steps(2, lambda n: n % 2 == 0) - 11,                   # the last slice: a full step, then 5 rows
                "per2_full": 32 * S,
                "per3_ragged": 16 * steps(3, lambda n: n % 3 == 0) - 15,                   # one row behind two full steps of its slice
                "per4": 64 * S,
                "per5_wrap": 16 * steps(5, lambda n: n % 5 != 0),                          # the last slice shorter than the others
                "per6": 16 * steps(6, lambda n: n >= 5 * S + 2)}
    # (S >= num_cus / 8, so every one of the first four passes batched_ring_ok; the fifth is the largest count that does not)
    return {"ring_1_group": 16 * S, "ring_1_and_2_groups": 16 * (S + 1), "ring_2_groups": 32 * S, "ring_uneven": 16 * (4 * S + 1),
            "layer_by_layer_ring": max(16, 16 * (num_cus // 8 - 1)), "layer_by_layer_vec": 185}


LIST_P = 2048
LIST_LIVE = (0, 1, 2, 17, 64)


def live_tiles_of(n_live, n_tiles=LIST_P // 32):
    """A spread-out ascending live set of n_live of n_tiles tiles that keeps the first and the last tile where it can."""
    if n_live == 0:
        return []
    if n_live == 1:
        return [n_tiles // 3]
    return sorted({round(i * (n_tiles - 1) / (n_live - 1)) for i in range(n_live)})


# ------------------------------------------------------------------------------------------------ markers
def marker_classes(P, slices, live_tiles=None):
    """{class name: point row} of the marker rows that exist at this point count, from the 16-point unit ranges `slices` of one job.
    With a live-tile list the units are the halves of the live tiles and a unit's first row comes from the list."""
    def row0(unit):
        return 16 * unit if live_tiles is None else 32 * live_tiles[unit // 2] + 16 * (unit % 2)
    n_units = (P + 15) // 16 if live_tiles is None else 2 * len(live_tiles)
    nonempty = [(a, b) for a, b in slices if a < b]
    out = {}
    if not nonempty:
        return out
    picks = {"first_slice": nonempty[0], "last_slice": nonempty[-1]}
    if len(nonempty) >= 3:
        picks["middle_slice"] = nonempty[len(nonempty) // 2]
    for name, (a, b) in picks.items():
        out[name + "_first_row"] = row0(a)
        out[name + "_last_row"] = min(row0(b - 1) + 15, P - 1)
    # the slice with the most steps (the first one has `per` of them): rows 0 and 15 of its first six steps, both half-waves of one
    a, b = max(nonempty, key=lambda r: r[1] - r[0])
    for k in range(min(6, b - a)):
        out[f"step{k}_row0"] = row0(a + k)
        if row0(a + k) + 15 < P:
            out[f"step{k}_row15"] = row0(a + k) + 15
    mid = a + (b - a) // 2
    for g in (0, 1):
        if row0(mid) + 8 * g + 3 < P:
            out[f"halfwave{g}"] = row0(mid) + 8 * g + 3
    if live_tiles is None:
        out["last_existing_row"] = P - 1
        if P % 16:
            out["ragged_step_first_row"] = 16 * (n_units - 1)
    else:
        for name, t in (("first_live_tile", live_tiles[0]), ("last_live_tile", live_tiles[-1])):
            out[name + "_low_half"] = 32 * t + 5
            out[name + "_high_half"] = 32 * t + 21
    assert all(0 <= r < P for r in out.values()), (P, out)
    return out


def marker_sets(classes, per_set=8):
    """The class rows, in ascending order, in sets of at most `per_set` rows."""
    rows = sorted(set(classes.values()))
    return [rows[i:i + per_set] for i in range(0, len(rows), per_set)]


# the classes some dense-form count of a precision must hit (asserted with the device's CU count)
DENSE_CLASSES = ["first_slice_first_row", "first_slice_last_row", "last_slice_first_row", "last_slice_last_row", "middle_slice_first_row",
                 "middle_slice_last_row", "halfwave0", "halfwave1", "last_existing_row"] + \
                [f"step{k}_row{r}" for k in range(6) for r in (0, 15)]
RAGGED_CLASSES = ["ragged_step_first_row"]                       # bf16x3 only: the fp32 ring takes whole groups
LIST_CLASSES = [f"{t}_live_tile_{h}_half" for t in ("first", "last") for h in ("low", "high")]


def bf16x3_regimes(P, n_jobs, num_cus):
    """The slice regimes of the dense bf16x3 launch at P, as a set of names (what the coverage assertions count)."""
    sl = bf16x3_slices(P, n_jobs, num_cus)
    lens = [b - a for a, b in sl]
    nonempty = [l for l in lens if l > 0]
    out = {f"slice_of_{l}_steps" for l in set(nonempty)}
    if len(set(nonempty)) > 1:
        out.add("slice_shorter_than_its_neighbours")
    if len(nonempty) < len(lens):
        out.add("empty_slices_behind_non_empty_ones")
    if P % 16 and nonempty[-1] > 1:
        out.add("ragged_last_step_behind_full_steps")
    if P % 16:
        out.add("ragged_last_step")
    return out


def ring_regimes(slices):
    return {f"slice_of_{b - a}_groups" for a, b in slices}


def check_coverage(C):
    """Every regime and marker class the GPU test is meant to visit is visited, for a device of C compute units (C >= 64)."""
    list_seen = set()
    for dens in (False, True):
        n_jobs = n_big_jobs(dens)
        # ---- bf16x3: slices of 1 .. 6 steps, a shorter slice, empty slices behind non-empty ones, a ragged step behind full ones
        counts = backward_counts("f32x", dens, C)
        seen = set()
        for regime, P in counts.items():
            seen |= bf16x3_regimes(P, n_jobs, C)
        want = {f"slice_of_{k}_steps" for k in range(1, 7)} | {"slice_shorter_than_its_neighbours", "empty_slices_behind_non_empty_ones",
                                                               "ragged_last_step_behind_full_steps", "ragged_last_step"}
        assert want <= seen, (dens, sorted(want - seen))
        assert bf16x3_regimes(counts["per2_one_step_slice"], n_jobs, C) >= {"slice_of_1_steps", "slice_of_2_steps", "empty_slices_behind_non_empty_ones"}
        assert "ragged_last_step_behind_full_steps" in bf16x3_regimes(counts["per3_ragged"], n_jobs, C)
        assert bf16x3_regimes(counts["per5_wrap"], n_jobs, C) >= {"slice_of_5_steps", "slice_shorter_than_its_neighbours"}
        classes = set()
        for P in counts.values():
            classes |= set(marker_classes(P, bf16x3_slices(P, n_jobs, C)))
        assert set(DENSE_CLASSES + RAGGED_CLASSES) <= classes, sorted(set(DENSE_CLASSES + RAGGED_CLASSES) - classes)
        # ---- fp32: batched ring slices of 1, 1 and 2, 2 groups and uneven ones; layer by layer on the ring and off it
        counts = backward_counts("f32", dens, C)
        fam = {r: big_job_slices("f32", P, n_jobs, C) for r, P in counts.items()}
        assert [fam[r][0] for r in counts] == ["ring_batched"] * 4 + ["ring_single", "vec_plain"]
        assert ring_regimes(fam["ring_1_group"][1]) == {"slice_of_1_groups"}
        assert ring_regimes(fam["ring_1_and_2_groups"][1]) == {"slice_of_1_groups", "slice_of_2_groups"}
        assert ring_regimes(fam["ring_2_groups"][1]) == {"slice_of_2_groups"}
        assert len(ring_regimes(fam["ring_uneven"][1])) == 2
        classes = set()
        for r, P in counts.items():
            classes |= set(marker_classes(P, fam[r][1]))
        assert set(DENSE_CLASSES) <= classes, sorted(set(DENSE_CLASSES) - classes)
        # ---- list form: 0, 1 and 2 groups per fp32 slice, both halves of the first and the last live tile
        for n_live in LIST_LIVE:
            tiles = live_tiles_of(n_live)
            assert len(tiles) == n_live and tiles == sorted(set(tiles)) and all(0 <= t < LIST_P // 32 for t in tiles)
            list_seen |= ring_regimes(batched_ring_slices(LIST_P, n_jobs, C, n_live))
            if n_live:
                for prec in ("f32", "f32x"):
                    got = set(marker_classes(LIST_P, big_job_slices(prec, LIST_P, n_jobs, C, n_live)[1], tiles))
                    assert set(LIST_CLASSES) <= got
    assert {"slice_of_0_groups", "slice_of_1_groups", "slice_of_2_groups"} <= list_seen
    assert live_tiles_of(64) == list(range(64)) and live_tiles_of(2) == [0, 63]
    # ---- the integer probes reach every row of the table, and the ring rows in both forms
    rows = set()
    for name, layout in probe_layouts().items():
        (ldz, zc0, n_out), (ldh, hc0, n_in), _, _ = layout
        for P, form in probe_counts(layout, C):
            row, got = wgrad_form(n_out, n_in, ldz, zc0, ldh, hc0, P, C)
            assert got == form, (name, P, got, form)
            rows.add((row, form))
    assert {(r, PLAIN) for r in range(len(WG_ROWS))} | {(r, RING) for r in range(1, 6)} | {(None, RING256)} <= rows
    groups = [len(ring_regimes(small_ring_slices(P, C))) for P in ring_counts(C)]
    assert groups.count(1) >= 4 and groups.count(2) >= 2                      # even splits, and the uneven ones



# ------------------------------------------------------------------------------------------------ truth and bound
def truth_and_bound(dz, hin, extra, per_row=1):
    """From the fp32 operands dz [n, n_out] and hin [n, n_in] (any device) -> (truth, bound), float64 [n_out, n_in]: dz^T hin and
    (per_row n + extra) u sum_p |dz hin| with n, per element, the number of rows whose term is not zero."""
    d, h = dz.double(), hin.double()
    truth = d.T @ h
    mag = d.abs().T @ h.abs()
    n = (d != 0).double().T @ (h != 0).double()
    return truth, (per_row * n + extra) * U * mag


def colsum_and_bound(dz, extra=1):
    """-> (truth, bound), float64 [n_out]: the column sums of dz and (n + extra) u sum_p |dz|, n the non-zero rows of the column."""
    d = dz.double()
    return d.sum(0), ((d != 0).double().sum(0) + extra) * U * d.abs().sum(0)


F32_DW = dict(extra=2, per_row=1)
BF16X3_DROPPED = 17                      # ceil((2^-20 + 2^-27) / u) = ceil(16.125)
BF16X3_DW = dict(extra=2 + BF16X3_DROPPED, per_row=6)

# ------------------------------------------------------------------------------------------------ bf16 split


def _truncate_bf16(x):
    return (x.view(torch.int32) & -65536).view(torch.float32)


def split3_bf16(x):
    """split3_bf16 of csrc/nerf_wgrad_bf16x3.hip.inc on a float32 tensor -> (hi, mid, lo), each a bf16 value held in float32."""
    assert x.dtype == torch.float32
    hi = _truncate_bf16(x)
    r1 = x - hi
    mid = _truncate_bf16(r1)
    r2 = r1 - mid
    return hi, mid, _truncate_bf16(r2)


DROPPED_PRODUCT_BOUND = 2.0 ** -20 + 2.0 ** -27


def dropped_products(a, b):
    """float64 |mid_a lo_b + lo_a mid_b + lo_a lo_b| / |a b| of float32 tensors a, b (no zeros)."""
    (_, ma, la), (_, mb, lb) = split3_bf16(a), split3_bf16(b)
    ma, la, mb, lb = ma.double(), la.double(), mb.double(), lb.double()
    return (ma * lb + la * mb + la * lb).abs() / (a.double() * b.double()).abs()


# ------------------------------------------------------------------------------------------------ figures
def parity_record(key, stats):
    """Keep the measured figures: merged into profiles/wgrad_bounds.json.  Where NERF_PARITY_COPY_DIR names a directory (a run on a
    machine whose working tree does not come back), a copy of the file goes there as well."""
    rec = {}
    if os.path.exists(BOUNDS_JSON):
        with open(BOUNDS_JSON) as f:
            rec = json.load(f)
    rec[key] = stats
    os.makedirs(os.path.dirname(BOUNDS_JSON), exist_ok=True)
    with open(BOUNDS_JSON, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    out = os.environ.get("NERF_PARITY_COPY_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        shutil.copyfile(BOUNDS_JSON, os.path.join(out, os.path.basename(BOUNDS_JSON)))
