"""The deformation field of include/nerf_mi355x_deform.h restated in numpy (test infrastructure, no test in here).

Two forms of the same formulas: dtype = np.float32 performs every operation of the header in its order with its own rounding (numpy
rounds each elementwise fp32 operation once), so the forward is the kernels' bits; dtype = np.float64 is the yardstick of the table
gradient.  Also the index function of the packed device layout.  `t` is the frame number PER ROW here: a caller with rays expands
time[id // n_samples] itself."""
import numpy as np

F = 64


def packed_index(i, j, y, c, f, T, R):
    """Where feat[i][j, f, y, c] lies in `packed`: channel innermost, one tap of one plane is one row of 64 floats."""
    return (((i * 3 + j) * T + y) * R + c) * F + f


def pack(feat):
    """Three tables [3, 64, T, R] -> packed [9 * T * R * 64], by the index function (no arithmetic)."""
    return np.ascontiguousarray(np.stack(feat).transpose(0, 1, 3, 4, 2)).reshape(-1)


def unpack(packed, T, R):
    """packed [9 * T * R * 64] -> three tables [3, 64, T, R]."""
    full = packed.reshape(3, 3, T, R, F).transpose(0, 1, 4, 2, 3)
    return [np.ascontiguousarray(full[i]) for i in range(3)]


def _geometry(x, t, T, R, dtype):
    one = dtype(1)
    tc = np.minimum(np.maximum(np.where(np.isnan(t), dtype(0), t), dtype(0)), dtype(T - 1)).astype(dtype)
    y0 = np.minimum(np.floor(tc).astype(np.int64), T - 2)
    wy = (tc - y0.astype(dtype)).astype(dtype)
    uy = (one - wy).astype(dtype)
    x0, wx, ux = [], [], []
    for j in range(3):
        ix = (x[:, j] * dtype(R - 1)).astype(dtype)
        c = np.clip(np.floor(ix).astype(np.int64), 0, R - 2)
        w = (ix - c.astype(dtype)).astype(dtype)
        x0.append(c), wx.append(w), ux.append((one - w).astype(dtype))
    return y0, wy, uy, x0, wx, ux


def _values(feat, geom, dtype):
    """v[i][j] [n, 64]: the four-tap bilinear value of every plane at every row."""
    y0, wy, uy, x0, wx, ux = geom
    v = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            P = feat[i][j].astype(dtype)                                  # [64, T, R]
            a00, a01 = P[:, y0, x0[j]].T, P[:, y0, x0[j] + 1].T           # [n, 64]
            a10, a11 = P[:, y0 + 1, x0[j]].T, P[:, y0 + 1, x0[j] + 1].T
            top = a00 * ux[j][:, None] + a01 * wx[j][:, None]
            bot = a10 * ux[j][:, None] + a11 * wx[j][:, None]
            v[i][j] = top * uy[:, None] + bot * wy[:, None]
    return v


def _fold(p):
    """The sum over the 64 channels in the header's order: p[f] += p[f + h], h = 32, 16, 8, 4, 2, 1."""
    for h in (32, 16, 8, 4, 2, 1):
        p = p[:, :h] + p[:, h:2 * h]
    return p[:, 0]


def deform(x, t, feat, dtype=np.float32):
    """x [n, 3] in [0, 1], t [n] frame numbers, feat: three [3, 64, T, R] -> (delta [n, 3], x_warped [n, 3]) in `dtype`."""
    x, t = np.asarray(x, dtype=dtype), np.asarray(t, dtype=dtype)
    T, R = feat[0].shape[2], feat[0].shape[3]
    v = _values(feat, _geometry(x, t, T, R, dtype), dtype)
    delta = np.stack([_fold((v[i][0] * v[i][1]) * v[i][2]) for i in range(3)], axis=1).astype(dtype)
    nan_t = np.isnan(t)
    delta[nan_t] = np.nan
    warped = np.minimum(np.maximum(x + delta, dtype(0)), dtype(1)).astype(dtype)
    warped = np.where((t == 0)[:, None], x, warped)
    warped[nan_t] = np.nan
    return delta, warped


def table_gradient(x, t, feat, g_x_warped=None, g_delta=None, dtype=np.float64):
    """The gradient of  sum(x_warped * g_x_warped) + sum(delta * g_delta)  with respect to the three tables, by the header's formulas;
    rows are added one after the other in `dtype` (np.add.at).  -> three arrays [3, 64, T, R]."""
    x, t = np.asarray(x, dtype=dtype), np.asarray(t, dtype=dtype)
    T, R = feat[0].shape[2], feat[0].shape[3]
    geom = _geometry(x, t, T, R, dtype)
    y0, wy, uy, x0, wx, ux = geom
    v = _values(feat, geom, dtype)
    delta, _ = deform(x, t, feat, dtype)
    s = x + delta
    with np.errstate(invalid="ignore"):
        gate = ((t != 0) & ~np.isnan(t))[:, None] & (s >= 0) & (s <= 1)
    g = np.zeros_like(x)
    if g_x_warped is not None:
        g = np.where(gate, np.asarray(g_x_warped, dtype=dtype), dtype(0))
    if g_delta is not None:
        g = (g + np.asarray(g_delta, dtype=dtype)).astype(dtype)
    g[np.isnan(t)] = 0
    out = [np.zeros((3, F, T, R), dtype=dtype) for _ in range(3)]
    for i in range(3):
        for j in range(3):
            a, b = [k for k in range(3) if k != j]
            q = g[:, i, None] * (v[i][a] * v[i][b])                        # [n, 64]
            qt, qb = q * uy[:, None], q * wy[:, None]
            G = out[i][j]
            np.add.at(G, (slice(None), y0, x0[j]), (qt * ux[j][:, None]).T)
            np.add.at(G, (slice(None), y0, x0[j] + 1), (qt * wx[j][:, None]).T)
            np.add.at(G, (slice(None), y0 + 1, x0[j]), (qb * ux[j][:, None]).T)
            np.add.at(G, (slice(None), y0 + 1, x0[j] + 1), (qb * wx[j][:, None]).T)
    return out


def gate(x, t, feat, dtype=np.float64):
    """(s = x + delta [n, 3], open [n, 3]): what the clamp sees and where the gradient of x_warped reaches delta."""
    x, t = np.asarray(x, dtype=dtype), np.asarray(t, dtype=dtype)
    delta, _ = deform(x, t, feat, dtype)
    s = x + delta
    with np.errstate(invalid="ignore"):
        return s, ((t != 0) & ~np.isnan(t))[:, None] & (s >= 0) & (s <= 1)
