"""float64 restatement of the fp16-activation MLP (csrc/nerf_mlp_f16s.hip.inc, csrc/nerf_mlp_f16.hip.inc), written from its rounding
points, and a builder of networks and points on which every product and partial sum is an exact small number.  Pure torch on the
CPU; it imports the oracle and nothing of the package.  The yardstick of tests/test_gpu_f16_exact.py and tests/test_gpu_f16_floor.py,
itself checked by tests/test_f16_reference_cpu.py.

The rounding points of both kernels (gemm16s_layer / the `(_Float16)acc` epilogues, and the head code at their ends):
    encodings   computed in fp32, stored as fp16
    weights     fp16; biases fp32 (the C operand of a tile's first MFMA)
    pts_linears.0..7, feature_linear (no ReLU), views_linears.0:  fp32 accumulator -> fp16 (round to nearest even) -> ReLU
    alpha_linear, rgb_linear:  fp32 sums over the fp16 activations plus the fp32 bias, written as they are
"""
import json
import os
import shutil

import torch

import nerf_oracle as oracle

U = 2.0 ** -24
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(REPO, "profiles", "f16_parity.json")


def model_of(prefix):
    return "fine" if prefix == "model_fine" else ""


def _to_f16(z, toward_zero):
    """float64 -> fp32 -> fp16, round to nearest even both times (torch's casts); `toward_zero` truncates the second step instead:
    where the nearest fp16 is larger in magnitude than the fp32 value, one step of the fp16 bit pattern back towards zero."""
    z32 = z.to(torch.float32)
    h = z32.half()
    if toward_zero:
        bits = h.view(torch.int16)
        away = h.float().abs() > z32.abs()
        h = torch.where(away, bits - 1, bits).view(torch.float16)
    return h


def emulate(sd, prefix, pts, dirs, accumulate=torch.float64, drop_bias=None, toward_zero=False, swap_slots=None):
    """The fp16 kernels' arithmetic on fp32 points [P,3] and directions [P,3] (one per point) -> dict of float64 tensors:
    raw [P,4] = (r, g, b, sigma), h7 [P,256] = relu of pts_linears.7 (what alpha_linear reads), views [P,128] (what rgb_linear reads).
    accumulate=torch.float32 is the second realisation: every dot product as a float32 matmul instead of a float64 one.
    Seeded faults, for the tests of the criteria:
      drop_bias=(layer, m)       the bias of the 16-feature out-tile m of that hidden layer is not added
      toward_zero=True           the fp32 -> fp16 step of every hidden layer truncates
      swap_slots=(layer, a, b)   the 8-wide k-slots a and b of that layer's input change places"""
    W = lambda n: sd[f"{prefix}.{n}.weight"].half().to(accumulate)
    B = lambda n: sd[f"{prefix}.{n}.bias"].to(accumulate)

    def dense(x16, name):
        if swap_slots is not None and swap_slots[0] == name:
            a, b = 8 * swap_slots[1], 8 * swap_slots[2]
            x16 = x16.clone()
            x16[:, a:a + 8], x16[:, b:b + 8] = x16[:, b:b + 8].clone(), x16[:, a:a + 8].clone()
        bias = B(name)
        if drop_bias is not None and drop_bias[0] == name:
            bias = bias.clone()
            bias[16 * drop_bias[1]:16 * drop_bias[1] + 16] = 0
        return x16.to(accumulate) @ W(name).T + bias

    def hidden(x16, name, relu=True):
        h = _to_f16(dense(x16, name).double(), toward_zero)
        return torch.relu(h) if relu else h

    pe = oracle.freq_encode(pts.float(), oracle.XYZ_FREQS).half()
    de = oracle.freq_encode(dirs.float(), oracle.DIR_FREQS).half()
    h = pe
    for i in range(8):
        h = hidden(h, f"pts_linears.{i}")
        if i == 4:
            h = torch.cat([pe, h], -1)
    feat = hidden(h, "feature_linear", relu=False)
    views = hidden(torch.cat([feat, de], -1), "views_linears.0")
    sigma = dense(h, "alpha_linear").double()
    rgb = dense(views, "rgb_linear").double()
    return dict(raw=torch.cat([rgb, sigma], -1), h7=h.double(), views=views.double())


def weights_f16(sd, prefix):
    """The sub-model with its weights rounded to fp16 (kept in fp32 storage) and its biases as they are."""
    return {k: (v.half().float() if k.endswith("weight") else v) for k, v in sd.items() if k.startswith(prefix + ".")}


def truth16(sd, prefix, pts, dirs):
    """What the fp16 kernels approximate: the network with fp16-rounded weights, encodings and layers in float64 -> [P,4] float64
    (the oracle rounds its result to fp32: 6e-8 relative, three orders below anything compared against it)."""
    with torch.no_grad():
        return oracle.network_forward(weights_f16(sd, prefix), pts[:, None, :], dirs, model_of(prefix), mlp_dtype=torch.float64)[:, 0].double()


def head_magnitude(sd, prefix, E):
    """Sum_k |w_k h_k| + |b| of the four outputs, from an emulation's own last activations and the fp16-rounded head weights -> [P,4]."""
    w = lambda n: sd[f"{prefix}.{n}.weight"].half().double().abs()
    b = lambda n: sd[f"{prefix}.{n}.bias"].double().abs()
    return torch.cat([E["views"].abs() @ w("rgb_linear").T + b("rgb_linear"), E["h7"].abs() @ w("alpha_linear").T + b("alpha_linear")], -1)


HEAD_K = torch.tensor([128.0, 128.0, 128.0, 256.0], dtype=torch.float64)


def floor_figures(got, E, T, magnitude):
    """The three criteria of the rounding floor for outputs `got` [P,4] against the emulation E (its raw), the truth T and the head
    magnitudes of E -> dict of figures and the three verdicts.
      share      of the points with all four outputs within (K + 2) u (sum|w h| + |b|) of E's: no hidden rounding flipped   (>= min_share)
      max_over_M max_p |got - E| / M_c per channel, M_c = max_p |E - T|: both are realisations of one rounding process around T  (<= 2)
      rms_ratio  rms_p(got - T) / rms_p(E - T) per channel: the same amount of noise                                             (<= 1.25)"""
    got, T = got.double(), T.double()
    d = (got - E).abs()
    share = (d <= (HEAD_K + 2) * U * magnitude).all(-1).double().mean().item()
    M = (E - T).abs().max(0).values
    rms = lambda x: x.pow(2).mean(0).sqrt()
    rng = T.abs().max(0).values
    return dict(share=share, max_over_M=(d.max(0).values / M).tolist(), rms_ratio=(rms(got - T) / rms(E - T)).tolist(),
                M_over_range=(M / rng).tolist(), max_over_range=(d.max(0).values / rng).tolist(), rms_floor_over_range=(rms(E - T) / rng).tolist())


def floor_verdicts(fig, min_share):
    return dict(share=fig["share"] >= min_share, max=max(fig["max_over_M"]) <= 2.0, rms=max(fig["rms_ratio"]) <= 1.25)


# ------------------------------------------------------------------------------------------------ exact probes
def _allowed_xyz(zero_axis):
    return [0, 1, 2] + [3 + 6 * k + zero_axis for k in range(oracle.XYZ_FREQS)] + [6 + 6 * k + zero_axis for k in range(oracle.XYZ_FREQS)]


def _allowed_dir(zero_axis):
    return [0, 1, 2] + [3 + 6 * k + zero_axis for k in range(oracle.DIR_FREQS)] + [6 + 6 * k + zero_axis for k in range(oracle.DIR_FREQS)]


def probe_points(seed, zero_axis, n):
    """n points on the 1/4 grid of [-4, 4]^3 and directions on the 1/2 grid of [-2, 2]^3, both 0 on `zero_axis`: there every sin is
    exactly 0 and every cos exactly 1, in torch and in the kernels' sincos_cw with its angle doubling alike."""
    g = torch.Generator().manual_seed(1000 + 10 * seed + zero_axis)
    pts = torch.randint(-16, 17, (n, 3), generator=g).float() / 4
    dirs = torch.randint(-4, 5, (n, 3), generator=g).float() / 2
    pts[:, zero_axis] = 0
    dirs[:, zero_axis] = 0
    return pts, dirs


def probe_rays(gen, zero_axis, n_rays, S, per_ray):
    """Rays whose points and unit directions are exact: o on the 1/4 grid with o[zero_axis] = 0, d = +-e_j * {1, 2, 4} for an axis
    j != zero_axis (d / ||d|| is exactly +-e_j), depths multiples of 1/4 in [0, 1] and |o_j| <= 4 - |d|, so o + d t stays in [-4, 4].
    The other free coordinate takes four values, which keeps the distinct (point, direction) pairs of a network below 600.
    -> o [n,3], d [n,3], t ([n,S] per ray, [S] shared), points [n,S,3], unit directions [n,3]."""
    free = [a for a in range(3) if a != zero_axis]
    pick = torch.randint(0, 2, (n_rays,), generator=gen)
    j = torch.tensor(free)[pick]
    k = torch.tensor(free)[1 - pick]
    scale = 2.0 ** torch.randint(0, 3, (n_rays,), generator=gen).float()
    sign = torch.randint(0, 2, (n_rays,), generator=gen).float() * 2 - 1
    rows = torch.arange(n_rays)
    d = torch.zeros(n_rays, 3)
    d[rows, j] = sign * scale
    o = torch.zeros(n_rays, 3)
    span = (4 - scale) * 4                                            # |o_j| <= 4 - |d| in quarter steps
    o[rows, j] = torch.floor((torch.rand(n_rays, generator=gen) * 2 - 1) * span).clamp(-span, span) / 4
    o[rows, k] = torch.tensor([-2.75, -0.25, 1.5, 3.0])[torch.randint(0, 4, (n_rays,), generator=gen)]
    t = torch.sort(torch.randint(0, 5, (n_rays if per_ray else 1, S), generator=gen).float() / 4, dim=-1).values
    unit = torch.zeros(n_rays, 3)
    unit[rows, j] = sign
    pts = o[:, None, :] + d[:, None, :] * t[:, :, None]              # exact in fp32
    assert pts.abs().max() <= 4 and torch.all(pts[..., zero_axis] == 0)
    return o, d, (t if per_ray else t[0]).contiguous(), pts, unit


def probe_network(seed, zero_axis):
    """A sub-model (24 tensors, keys without prefix) of +-1 weights and small integer biases: every row holds two +1 and two -1 (the
    two heads: four and four) at seeded columns; layer 0, the skip part of layer 5 and the direction part of the views layer use
    only the raw columns and the sin / cos columns of `zero_axis`, so every other encoding entry meets a zero.  The bias of
    alpha_linear is minus the median of sigma over probe_points(seed, zero_axis, 1024), so that both signs occur."""
    g = torch.Generator().manual_seed(7919 * seed + zero_axis)
    xyz, dr = _allowed_xyz(zero_axis), _allowed_dir(zero_axis)
    cols = {"pts_linears.0": xyz, "pts_linears.5": xyz + list(range(63, 319)), "views_linears.0": list(range(256)) + [256 + c for c in dr]}
    sub = {}
    for name in [k[:-7] for k in oracle.SUBMODEL_KEYS if k.endswith(".weight")]:
        n_out, n_in = oracle.SUBMODEL_SHAPES[name + ".weight"]
        allowed = torch.tensor(cols.get(name, list(range(n_in))))
        nnz = 8 if name in ("alpha_linear", "rgb_linear") else 4
        w = torch.zeros(n_out, n_in)
        for r in range(n_out):
            pick = allowed[torch.randperm(len(allowed), generator=g)[:nnz]]
            w[r, pick[:nnz // 2]] = 1.0
            w[r, pick[nnz // 2:]] = -1.0
        sub[name + ".weight"] = w
        sub[name + ".bias"] = torch.randint(-2, 3, (n_out,), generator=g).float()
    sub["alpha_linear.bias"] = torch.zeros(1)
    pts, dirs = probe_points(seed, zero_axis, 1024)
    sigma = probe_forward(sub, pts, dirs)[:, 3]
    sub["alpha_linear.bias"] = -torch.median(sigma).reshape(1).float()
    return {k: sub[k].contiguous() for k in oracle.SUBMODEL_KEYS}


def both_models(sub):
    """The 48-tensor state dict with `sub` as its coarse and its fine model."""
    return {f"{m}.{k}": v.clone() for m in ("model", "model_fine") for k, v in sub.items()}


def probe_forward(sub, pts, dirs, dtype=torch.float64):
    """The oracle on a probe sub-model, one direction per point -> raw [P,4] float32."""
    with torch.no_grad():
        return oracle.network_forward({f"model.{k}": v for k, v in sub.items()}, pts[:, None, :], dirs, "", mlp_dtype=dtype)[:, 0]


def repeated(n, n_distinct, seed):
    """Row ids of an n-row arrangement of n_distinct rows: whole seeded permutations one after another, the last one cut."""
    g = torch.Generator().manual_seed(seed)
    reps = -(-n // n_distinct)
    return torch.cat([torch.randperm(n_distinct, generator=g) for _ in range(reps)])[:n]


N_MANY = 2 * 256 * 256 + 3 * 256 + 77          # 131 917 points: every one of <= 256 persistent workgroups walks two or three 256-point tiles


def parity_record(section, key, stats):
    """Keep the measured figures: merged into profiles/f16_parity.json.  Where NERF_PARITY_COPY_DIR names a directory (a run on a
    machine whose working tree does not come back), a copy of the file goes there as well."""
    rec = {}
    if os.path.exists(PARITY_JSON):
        with open(PARITY_JSON) as f:
            rec = json.load(f)
    rec.setdefault(section, {})[key] = stats
    os.makedirs(os.path.dirname(PARITY_JSON), exist_ok=True)
    with open(PARITY_JSON, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    out = os.environ.get("NERF_PARITY_COPY_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        shutil.copyfile(PARITY_JSON, os.path.join(out, os.path.basename(PARITY_JSON)))


# ------------------------------------------------------------------------------------------------ shared cases
PROBES = tuple((seed, zero_axis) for zero_axis in range(3) for seed in range(3))          # nine networks; the conditions hold for each
FLOOR_CASES = (("base", "model"), ("base", "model_fine"), ("white", "model_fine"), ("trained", "model_fine"))
N_FLOOR = 4113                                  # 17 tiles of 256 points, the last one ragged


def floor_points():
    """The first 4113 merged sample points of tests/golden/sampling.npz, each with its ray's normalised direction."""
    import numpy as np
    with np.load(os.path.join(REPO, "tests", "golden", "sampling.npz")) as z:
        o, d, t = (torch.from_numpy(z[k]) for k in ("rays_o", "rays_d", "t_sorted"))
    pts = (o[:, None, :] + d[:, None, :] * t[:, :, None]).reshape(-1, 3)[:N_FLOOR].contiguous()
    vd = (d / torch.norm(d, dim=-1, keepdim=True))[:, None, :].expand(-1, t.shape[1], 3).reshape(-1, 3)[:N_FLOOR].contiguous()
    return pts, vd
