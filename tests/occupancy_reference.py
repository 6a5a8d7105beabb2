"""NumPy restatement of the occupancy-grid definitions of DESIGN.md section 2.9 (include/nerf_mi355x.h, nerf_occupancy_*), for the
GPU tests to compare with byte for byte.  A helper, not a test.  Written from the definitions, not from the kernels: the
dilation is a separable running maximum here (the kernel scans the neighbourhood of every cell), the bits are packed with
np.packbits, and the lookup is float32 with every operation rounded on its own."""
import numpy as np


def cells(field, level, dilate):
    """bool [nx-1, ny-1, nz-1]: cell (i,j,k) is occupied iff a grid point in [i-r, i+1+r] x [j-r, j+1+r] x [k-r, k+1+r], clipped
    to the grid, has f > level or is NaN."""
    f = np.asarray(field, dtype=np.float32)
    assert f.ndim == 3 and min(f.shape) >= 2 and dilate >= 0
    with np.errstate(invalid="ignore"):
        hot = (f > np.float32(level)) | np.isnan(f)
    for axis in range(3):
        n = hot.shape[axis]
        src = np.moveaxis(hot, axis, 0)
        out = np.zeros((n - 1,) + src.shape[1:], dtype=bool)
        for i in range(n - 1):                                  # points i-r .. i+1+r of this axis
            out[i] = src[max(i - dilate, 0):min(i + 1 + dilate, n - 1) + 1].any(axis=0)
        hot = np.moveaxis(out, 0, axis)
    return hot


def pack(occupied):
    """Cell id (i*(ny-1) + j)*(nz-1) + k -> bit (id & 31) of 32-bit word (id >> 5); an even number of words, tail bits 0."""
    flat = np.ascontiguousarray(occupied, dtype=bool).reshape(-1)
    n_words = 2 * ((flat.size + 63) // 64)
    padded = np.zeros(n_words * 32, dtype=bool)
    padded[:flat.size] = flat
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def build(field, level, dilate):
    return pack(cells(field, level, dilate))


def lookup_frame(bbox, dims):
    """min = fp32(bbox min), inv = fp32((n - 1) / (max - min)): float64 on the host, rounded once."""
    b = np.asarray(bbox, dtype=np.float64).reshape(2, 3)
    return b[0].astype(np.float32), ((np.asarray(dims, dtype=np.float64) - 1.0) / (b[1] - b[0])).astype(np.float32)


def keep(o, d, t, words, dims, box_min, inv):
    """bool [n, S]: sample (ray r, depth t[r, s]) is kept iff it is outside the box, NaN, or in an occupied cell.
    o, d: [n, 3] float32; t: [n, S] or [S] float32 (a shared table)."""
    o, d = np.asarray(o, dtype=np.float32), np.asarray(d, dtype=np.float32)
    t = np.broadcast_to(np.asarray(t, dtype=np.float32), (o.shape[0], np.shape(t)[-1]))
    box_min, inv = np.asarray(box_min, dtype=np.float32), np.asarray(inv, dtype=np.float32)
    words = np.asarray(words, dtype=np.uint32)
    inside = np.ones(t.shape, dtype=bool)
    idx = []
    with np.errstate(all="ignore"):
        for a in range(3):
            x = o[:, a, None] + d[:, a, None] * t                # two float32 roundings
            c = np.floor((x - box_min[a]) * inv[a])
            assert x.dtype == np.float32 and c.dtype == np.float32
            ok = (c >= 0) & (c <= np.float32(dims[a] - 2))        # False for NaN
            inside &= ok
            idx.append(np.where(ok, c, 0).astype(np.int64))
    cell = (idx[0] * (dims[1] - 1) + idx[1]) * (dims[2] - 1) + idx[2]
    bit = (words[cell >> 5] >> (cell & 31).astype(np.uint32)) & 1
    return ~inside | (bit != 0)
