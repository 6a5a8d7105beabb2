"""What tests/test_gpu_train_chain_exact.py holds the training MLP pair to: the SAVE forwards (nerf_mlp_forward_rays_save*,
nerf_mlp_forward_points_save) and the data-gradient chain (csrc/nerf_mlp_bwd_f32.hip.inc, nerf_mlp_bwd_f32x.hip.inc) with the
direction adjoints behind it.  Pure torch on the CPU (every function also runs on device tensors); it imports the oracle and
tests/f16_reference.py and nothing of the package.  Checked by tests/test_train_chain_reference_cpu.py.

On the probe networks and points of f16_reference (+-1 weights, integer biases, points on the 1/4 grid with one zero axis) and an
integer d loss / d raw, every tensor the pair writes is a small multiple of 1/4 and every sum behind it stays below 2^24 units, so
the fp32 chain, the split-fp16 chain and float64 must agree BIT FOR BIT in any summation order.  The only inexact values are the
sin / cos of the two non-zero axes; the probe weights give them zero weight, so they reach nothing but their own pe / dpe columns
and the weight-gradient columns that multiply them (exact_masks: 22 528 of the 595 844 gradient elements, fixed by construction).

The backward is written rule by rule (network.py:49-74 under autograd):
    g_hv = g_rgb Wr            g_zv = g_hv * (zv > 0)        [g_f | g_dpe] = g_zv Wv
    g_h7 = g_f Wf + g_sigma w_alpha                           g_z(l) = g_h(l) * (z(l) > 0)
    g_h(l-1) = g_z(l) W(l)     layer 5: [g_pe | g_h4] = g_z5 W5               g_pe += g_z0 W0
    g_x = (d pe / d x)^T g_pe  g_t = g_x . rays_d            g_v = sum_s (d dpe / d v)^T g_dpe
    g_rays_d_view = (g_v - v (v . g_v)) / |d|                 dW = g_z^T input, db = sum_p g_z
`fault` seeds one wrong rule (FAULTS), for the test that the compared tensors notice it."""
import json
import os
import shutil

import torch

import f16_reference as R
import nerf_oracle as oracle
from wgrad_reference import PARAM_SHAPES, Grad, Save, pad32

REPO = R.REPO
EXACT_JSON = os.path.join(REPO, "profiles", "train_chain_exact.json")
TWO24 = float(2 ** 24)
GRID = 4.0                                   # every forward value is a multiple of 1 / GRID
CHAIN_MAX = 2 ** 11                          # the f32x chain keeps a value in one fp16 half under any power-of-two scale below this
DRAW_MAX = 4

FAULTS = ("mask_ge", "mask_other_tile", "alpha_dropped", "w5_parts_swapped", "row_duplicated", "g_t_unit_direction")
ROW_NAMES = ["gzv", "gf"] + [f"gz{l}" for l in range(8)]
SAVE_NAMES = ["pe", "dpe"] + [f"h{l}" for l in range(8)] + ["feature", "views"]


def integer_draw(P, seed):
    """d loss / d raw [P,4]: seeded integers in [-DRAW_MAX, DRAW_MAX]."""
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.randint(-DRAW_MAX, DRAW_MAX + 1, (P, 4), generator=g).float()


def _wb(sub, name, dtype):
    return sub[name + ".weight"].to(dtype), sub[name + ".bias"].to(dtype)


# ------------------------------------------------------------------------------------------------ forward
def forward(sub, pts, dirs, dtype=torch.float64):
    """The network on points [P,3] and per-point directions [P,3] (used as given) -> dict of `dtype` tensors: pe [P,64], dpe [P,32]
    (zero padded), z0..z7 / zv (pre-activations: the masks), h0..h7, feature, views, raw [P,4] = (r, g, b, sigma)."""
    lin = torch.nn.functional.linear
    P = pts.shape[0]
    pe63 = oracle.freq_encode(pts.to(dtype), oracle.XYZ_FREQS)
    de27 = oracle.freq_encode(dirs.to(dtype), oracle.DIR_FREQS)
    F = dict(pe=torch.cat([pe63, pe63.new_zeros(P, 1)], -1), dpe=torch.cat([de27, de27.new_zeros(P, 5)], -1))
    h = pe63
    for l in range(8):
        F[f"z{l}"] = lin(h, *_wb(sub, f"pts_linears.{l}", dtype))
        F[f"h{l}"] = h = torch.relu(F[f"z{l}"])
        if l == 4:
            h = torch.cat([pe63, h], -1)
    sigma = lin(h, *_wb(sub, "alpha_linear", dtype))
    F["feature"] = lin(h, *_wb(sub, "feature_linear", dtype))
    F["zv"] = lin(torch.cat([F["feature"], de27], -1), *_wb(sub, "views_linears.0", dtype))
    F["views"] = torch.relu(F["zv"])
    F["raw"] = torch.cat([lin(F["views"], *_wb(sub, "rgb_linear", dtype)), sigma], -1)
    return F


# ------------------------------------------------------------------------------------------------ backward
def encoding_backward(g_enc, x, n_freqs):
    """(d enc / d x)^T g_enc: column c is x_c, 3 + 6k + c is sin(2^k x_c), 6 + 6k + c is cos(2^k x_c) -> [P,3]."""
    g = g_enc[:, :3].clone()
    for k in range(n_freqs):
        f = 2.0 ** k
        g = g + f * (torch.cos(f * x) * g_enc[:, 3 + 6 * k:6 + 6 * k] - torch.sin(f * x) * g_enc[:, 6 + 6 * k:9 + 6 * k])
    return g


def encoding_backward_mag(g_enc, n_freqs):
    """The sum of absolute terms of encoding_backward with |sin|, |cos| <= 1 -> [P,3]."""
    g = g_enc[:, :3].abs()
    for k in range(n_freqs):
        g = g + 2.0 ** k * (g_enc[:, 3 + 6 * k:6 + 6 * k].abs() + g_enc[:, 6 + 6 * k:9 + 6 * k].abs())
    return g


def _abs_sum(a, b):
    """sum_k |a[.., k]| |b[k, ..]|: what an any-order product sum has to keep below 2^24 units."""
    return a.abs() @ b.abs()


def backward(sub, F, pts, dirs, draw, dtype=torch.float64, n_samples=1, rays_d=None, density_only=False, fault=None):
    """The adjoint of forward() for d loss / d raw = draw [P,4] -> dict of `dtype` tensors: gzv, gf, gz0..gz7, g_pe, g_x [P,3], g_v
    [n_rays,3] (= g_viewdirs of point mode: the direction as given, summed over the ray's n_samples consecutive points), and with
    rays_d [n_rays,3] (ray mode: x = o + d t, v = d / |d|) g_t [P] and g_rays_d_view [n_rays,3]; grads: the 24 parameter gradients;
    grad_mag: sum_p |dz| |input| of each; sum_mag: the largest sum of absolute terms of every other product sum, by name.
    density_only: the colour branch does not exist (its rows are absent, its gradients zero)."""
    assert fault is None or fault in FAULTS
    P = pts.shape[0]
    W = lambda n: sub[n + ".weight"].to(dtype)
    draw = draw.to(dtype)
    x, v = pts.to(dtype), dirs.to(dtype)
    live = lambda z: (z >= 0) if fault == "mask_ge" else (z > 0)
    if fault == "mask_other_tile":                                   # the mask bits of tile t taken from tile t ^ 1
        other = torch.arange(P) ^ 32
        other = torch.where(other < P, other, torch.arange(P))
        live = lambda z: (z > 0)[other]
    B, mag = {}, {}
    g_sigma = draw[:, 3:4]
    if density_only:
        g_f = draw.new_zeros(P, 256)
        g_dpe = draw.new_zeros(P, 27)
    else:
        g_hv = draw[:, :3] @ W("rgb_linear")
        B["gzv"] = g_hv * live(F["zv"])
        g_in = B["gzv"] @ W("views_linears.0")
        mag["g_hv"], mag["g_f"] = _abs_sum(draw[:, :3], W("rgb_linear")), _abs_sum(B["gzv"], W("views_linears.0"))
        B["gf"], g_dpe = g_in[:, :256], g_in[:, 256:]
        g_f = B["gf"]
    g_h = g_f @ W("feature_linear")
    if fault != "alpha_dropped":
        g_h = g_h + g_sigma @ W("alpha_linear")                      # the alpha term joins at z7
    mag["g_h7"] = _abs_sum(g_f, W("feature_linear")) + _abs_sum(g_sigma, W("alpha_linear"))
    g_pe = draw.new_zeros(P, 63)
    for l in range(7, -1, -1):
        B[f"gz{l}"] = g_h * live(F[f"z{l}"])
        g_in = B[f"gz{l}"] @ W(f"pts_linears.{l}")
        mag[f"g_in{l}"] = _abs_sum(B[f"gz{l}"], W(f"pts_linears.{l}"))
        if l == 5:                                                   # the skip: W5 = [pe | h4]
            g_pe_part, g_h = (g_in[:, 256:], g_in[:, :256]) if fault == "w5_parts_swapped" else (g_in[:, :63], g_in[:, 63:])
            g_pe = g_pe + g_pe_part
        elif l == 0:
            g_pe = g_pe + g_in
        else:
            g_h = g_in
    B["g_pe"] = g_pe
    B["g_x"] = encoding_backward(g_pe, x, oracle.XYZ_FREQS)
    mag["g_x"] = encoding_backward_mag(g_pe, oracle.XYZ_FREQS)
    n_rays = P // n_samples
    assert n_rays * n_samples == P
    B["g_v"] = encoding_backward(g_dpe, v, oracle.DIR_FREQS).view(n_rays, n_samples, 3).sum(1)
    mag["g_v"] = encoding_backward_mag(g_dpe, oracle.DIR_FREQS).view(n_rays, n_samples, 3).sum(1)
    if rays_d is not None:
        d = rays_d.to(dtype)
        norm = d.norm(dim=-1, keepdim=True)
        unit = d / norm
        d_pts = (unit if fault == "g_t_unit_direction" else d)[:, None, :].expand(n_rays, n_samples, 3).reshape(P, 3)
        B["g_t"] = (B["g_x"] * d_pts).sum(-1)
        mag["g_t"] = (mag["g_x"] * d_pts.abs()).sum(-1)
        B["g_rays_d_view"] = (B["g_v"] - unit * (unit * B["g_v"]).sum(-1, keepdim=True)) / norm
    if fault == "row_duplicated":                                    # the last point's rows also land on its neighbour
        for k in ROW_NAMES:
            if k in B:
                B[k] = B[k].clone()
                B[k][P - 2] = B[k][P - 1]
    # ---- parameter gradients, state_dict order
    h5_in = torch.cat([F["pe"][:, :63], F["h4"]], -1)
    inputs = [F["pe"][:, :63]] + [h5_in if l == 5 else F[f"h{l - 1}"] for l in range(1, 8)]
    pairs = [(B[f"gz{l}"], inputs[l]) for l in range(8)]
    if density_only:
        zero = lambda n_out, n_in: (draw.new_zeros(P, n_out), draw.new_zeros(P, n_in))
        pairs += [zero(128, 283), zero(256, 256), (g_sigma, F["h7"]), zero(3, 128)]
    else:
        pairs += [(B["gzv"], torch.cat([F["feature"], F["dpe"][:, :27]], -1)), (B["gf"], F["h7"]), (g_sigma, F["h7"]), (draw[:, :3], F["views"])]
    B["grads"], B["grad_mag"] = [], []
    for dz, hin in pairs:
        B["grads"] += [dz.T @ hin, dz.sum(0)]
        B["grad_mag"] += [dz.abs().T @ hin.abs(), dz.abs().sum(0)]
    assert [tuple(g.shape) for g in B["grads"]] == PARAM_SHAPES
    B["sum_mag"] = {k: float(m.max()) if m.numel() else 0.0 for k, m in mag.items()}
    return B


def reference(sub, pts, dirs, draw, dtype=torch.float64, **kw):
    """forward + backward in one dict."""
    F = forward(sub, pts, dirs, dtype)
    out = dict(F)
    out.update(backward(sub, F, pts, dirs, draw, dtype, **kw))
    return out


# ------------------------------------------------------------------------------------------------ what is exact, and the conditions
def exact_masks(zero_axis):
    """One bool tensor per parameter (state_dict order): False on the weight-gradient columns that multiply a sin / cos of a non-zero
    axis -- pts_linears.0, the first 63 columns of pts_linears.5, the last 27 of views_linears.0.  Fixed by the construction."""
    xyz = torch.zeros(63, dtype=torch.bool)
    xyz[R._allowed_xyz(zero_axis)] = True
    dr = torch.zeros(27, dtype=torch.bool)
    dr[R._allowed_dir(zero_axis)] = True
    out = [torch.ones(s, dtype=torch.bool) for s in PARAM_SHAPES]
    out[0][:, ~xyz] = False
    out[10][:, :63][:, ~xyz] = False
    out[16][:, 256:][:, ~dr] = False
    return out


def exact_columns(zero_axis):
    """-> (pe columns [64], dpe columns [32]) that are exact: the raw coordinates, the zero axis, the zero padding."""
    pe = torch.zeros(64, dtype=torch.bool)
    pe[R._allowed_xyz(zero_axis) + [63]] = True
    dpe = torch.zeros(32, dtype=torch.bool)
    dpe[R._allowed_dir(zero_axis) + [27, 28, 29, 30, 31]] = True
    return pe, dpe


N_EXEMPT, N_GRADIENT = 22528, 595844


def check_conditions(ref, masks):
    """The any-order conditions on a float64 reference: every compared value and every sum of absolute terms behind it is below 2^24
    units of its grid, and the chain values fit the f32x chain's hi half.  Asserts; -> the figures."""
    fig = {}
    for k in ROW_NAMES:
        if k in ref:
            assert torch.equal(ref[k], ref[k].round()), k
            fig[f"max|{k}|"] = float(ref[k].abs().max())
            assert fig[f"max|{k}|"] < CHAIN_MAX, (k, fig[f"max|{k}|"])
    for k, m in ref["sum_mag"].items():
        assert m < TWO24, (k, m)                                     # integer terms (g_x, g_t: products of integers)
    fig["max_sum_of_terms"] = max(ref["sum_mag"].values())
    worst = 0.0
    for g, m, keep in zip(ref["grads"], ref["grad_mag"], masks):     # dz is an integer, the input a multiple of 1 / GRID
        keep = keep.to(m.device)
        if keep.any():
            worst = max(worst, float((GRID * m)[keep].max()))
    assert worst < TWO24, worst
    fig["max_gradient_sum_of_terms_in_grid_units"] = worst
    return fig


# ------------------------------------------------------------------------------------------------ ReLU sign-bit blocks
def bits_blocks(ref, P, density_only=False):
    """The sign-bit blocks behind the saved rows (TrainSave::off_bits) -> (words, compared), int32 / bool [tiles, 9, 64, 4]: per
    32-point tile and masked tensor (0..7 = h0..h7, 8 = views) lane (p, hh) = p + 32 hh holds bit 16 (t & 1) + r of word t >> 1
    <-> activation 32 t + (r & 3) + 8 (r >> 2) + 4 hh of point p is > 0.  compared: lanes of points < P, the words a tensor has."""
    dev = ref["z0"].device
    tiles = pad32(P) // 32
    words = torch.zeros(tiles, 9, 64, 4, dtype=torch.int64, device=dev)
    compared = torch.zeros(tiles, 9, 64, 4, dtype=torch.bool, device=dev)
    lane = torch.arange(64, device=dev)
    pt, hh = lane & 31, lane >> 5
    point_ok = (torch.arange(tiles, device=dev)[:, None] * 32 + pt[None, :]) < P                         # [tiles, 64]
    r = torch.arange(16, device=dev)
    for which, key, ntile in [(l, f"z{l}", 8) for l in range(8)] + ([] if density_only else [(8, "zv", 4)]):
        pos = torch.zeros(tiles * 32, ref[key].shape[1], dtype=torch.bool, device=dev)
        pos[:P] = ref[key] > 0
        pos = pos.view(tiles, 32, -1)
        for t in range(ntile):
            feat = 32 * t + (r[None, :] & 3) + 8 * (r[None, :] >> 2) + 4 * hh[:, None]                 # [64, 16]
            got = pos[:, pt[:, None].expand(64, 16), feat].to(torch.int64)                              # [tiles, 64, 16]
            words[:, which, :, t >> 1] |= (got << (16 * (t & 1) + r)[None, None, :]).sum(-1)
        compared[:, which, :, :ntile // 2] = point_ok[:, :, None]
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return words, compared


# ------------------------------------------------------------------------------------------------ tiles
def tile_liveness(draw, density_only=False):
    """nerf_tile_flags_kernel's rule -> (bool per 32-point tile, count): a tile is live when any of its d loss / d raw rows is
    non-zero (density only: the sigma column alone).  P must be a multiple of 32."""
    nz = (draw[:, 3] != 0) if density_only else (draw != 0).any(-1)
    flags = nz.view(-1, 32).any(-1)
    return flags, int(flags.sum())


def arrange_dead_tiles(sigma, P, n_dead):
    """Point ids for a P-point call (a multiple of 32) whose first n_dead tiles hold no sigma > 0 and whose other tiles mix both
    signs, from the reference's sigma of a larger pool."""
    neg = (sigma <= 0).nonzero().flatten().tolist()
    pos = (sigma > 0).nonzero().flatten().tolist()
    assert len(neg) >= 32 * n_dead + (P - 32 * n_dead) // 2 and len(pos) >= (P - 32 * n_dead + 1) // 2
    rest_neg = neg[32 * n_dead:]
    return torch.tensor(neg[:32 * n_dead] + [(pos if i % 2 else rest_neg)[i // 2] for i in range(P - 32 * n_dead)])


# ------------------------------------------------------------------------------------------------ ray-mode inputs
def ray_case(seed, zero_axis, n_rays, S, per_ray):
    """f16_reference.probe_rays with a seed of its own -> dict(o, d, t, stride, pts [P,3], dirs [P,3] (unit, per point))."""
    gen = torch.Generator().manual_seed(977 * seed + 31 * zero_axis + 7 * n_rays + S + (1 if per_ray else 0))
    o, d, t, pts, unit = R.probe_rays(gen, zero_axis, n_rays, S, per_ray)
    return dict(o=o, d=d, t=t, stride=S if per_ray else 0, n_rays=n_rays, S=S, pts=pts.reshape(-1, 3).contiguous(),
                dirs=unit[:, None, :].expand(n_rays, S, 3).reshape(-1, 3).contiguous())


RAY_SHAPES = {1: (1, 1), 31: (31, 1), 32: (8, 4), 33: (11, 3), 127: (127, 1), 129: (43, 3), 185: (37, 5), 160: (40, 4), 192: (48, 4)}


def n_many(num_cus):
    """every one of <= num_cus persistent f32x workgroups walks two or three 128-point tiles; thousands of one-wave f32 workgroups"""
    return 2 * 128 * num_cus + 3 * 128 + 77


# ------------------------------------------------------------------------------------------------ figures
def exact_record(key, stats):
    """Keep the measured tallies: merged into profiles/train_chain_exact.json.  Where NERF_PARITY_COPY_DIR names a directory (a run
    on a machine whose working tree does not come back), a copy of the file goes there as well."""
    rec = {}
    if os.path.exists(EXACT_JSON):
        with open(EXACT_JSON) as f:
            rec = json.load(f)
    rec[key] = stats
    os.makedirs(os.path.dirname(EXACT_JSON), exist_ok=True)
    with open(EXACT_JSON, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    out = os.environ.get("NERF_PARITY_COPY_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        shutil.copyfile(EXACT_JSON, os.path.join(out, os.path.basename(EXACT_JSON)))

