"""CPU checks of the occupancy-grid feature (nerf_replication_amd/occupancy.py): properties of the NumPy
restatement tests/occupancy_reference.py on analytic fields, the argument checks of OccupancyGrid (before any library call) and
the size checks of the C entries.  The kernels are compared with the restatement in tests/test_gpu_occupancy.py."""
import numpy as np
import pytest
import torch

import isosurface_reference as R
import occupancy_reference as O

SHAPE = (9, 12, 17)


def _hot_corner(f, level):
    """bool per cell: one of its 8 corners is above the level (written with explicit slices, not with the restatement's scan)."""
    with np.errstate(invalid="ignore"):
        hot = f > np.float32(level)
    out = np.zeros(tuple(n - 1 for n in f.shape), dtype=bool)
    for o in range(8):
        di, dj, dk = (o >> 2) & 1, (o >> 1) & 1, o & 1
        out |= hot[di:f.shape[0] - 1 + di, dj:f.shape[1] - 1 + dj, dk:f.shape[2] - 1 + dk]
    return out


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_restatement_occupied_set_grows_with_dilate_and_covers_hot_corners(name):
    f, level = R.analytic_field(name, SHAPE), R.LEVELS[name]
    c0, c1, c2 = (O.cells(f, level, r) for r in (0, 1, 2))
    assert c0.shape == (8, 11, 16)
    assert np.array_equal(c0, _hot_corner(f, level))              # dilate 0: exactly the cells with a corner above the level
    assert c0.any() and not c2.all()
    assert (c1 | ~c0).all() and (c2 | ~c1).all()                  # monotone
    assert c1.sum() > c0.sum() and c2.sum() > c1.sum()
    # dilate r = dilate 0 of the cells within r cells (Chebyshev): one independent statement of the neighbourhood
    grown = np.zeros_like(c0)
    pad = np.pad(c0, 1)
    for di in range(3):
        for dj in range(3):
            for dk in range(3):
                grown |= pad[di:di + 8, dj:dj + 11, dk:dk + 16]
    assert np.array_equal(c1, grown)
    assert O.cells(f, level, 100).all()                           # clipped to the grid: everything once anything is hot


def test_restatement_nan_point_occupies_its_cells():
    f = np.full(SHAPE, -1.0, np.float32)
    assert not O.cells(f, 0.0, 0).any()
    f[4, 5, 6] = np.nan
    c = O.cells(f, 0.0, 0)
    assert c.sum() == 8 and c[3:5, 4:6, 5:7].all()
    assert O.cells(f, 0.0, 1).sum() == 64 and O.cells(f, 0.0, 1)[2:6, 3:7, 4:8].all()
    f[4, 5, 6] = 0.0                                              # a value equal to the level is not above it
    assert not O.cells(f, 0.0, 2).any()


@pytest.mark.parametrize("shape", [SHAPE, (2, 2, 2), (33, 33, 33), (5, 5, 6)])
def test_restatement_words_are_even_and_tail_bits_zero(shape):
    n_cells = (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
    words = O.build(np.ones(shape, np.float32), 0.0, 0)           # every cell occupied: the tail shows
    assert words.dtype == np.uint32 and len(words) % 2 == 0 and len(words) == 2 * ((n_cells + 63) // 64)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert bits[:n_cells].all() and not bits[n_cells:].any()
    f = R.analytic_field("random", shape)
    words = O.build(f, 0.5, 0)
    cells = O.cells(f, 0.5, 0).reshape(-1)
    for cid in (0, n_cells // 3, n_cells - 1):
        assert bool((words[cid >> 5] >> np.uint32(cid & 31)) & 1) == bool(cells[cid])


def test_restatement_keep():
    """Outside the box and NaN are kept; inside, the cell's bit decides; the cell of a point is the one that contains it."""
    dims, bbox = (5, 4, 3), [-1, -1, -1, 1, 2, 0]
    cells = np.zeros((4, 3, 2), dtype=bool)
    cells[2, 1, 0] = True
    words = O.pack(cells)
    lo, inv = O.lookup_frame(bbox, dims)
    assert lo.dtype == inv.dtype == np.float32 and np.array_equal(inv, np.array([2, 1, 2], np.float32))
    o = np.array([[0.25, 0.5, -0.75], [0.25, 0.5, -0.25], [5.0, 0.5, -0.75], [np.nan, 0.5, -0.75], [1.0, 0.5, -0.75]], np.float32)
    d = np.zeros_like(o)
    d[:, 0] = 1.0
    t = np.array([0.0, -0.5], np.float32)                         # the second sample moves one cell down in x
    k = O.keep(o, d, t, words, dims, lo, inv)
    assert k.tolist() == [[True, False], [False, False], [True, True], [True, True], [True, False]]   # x == max is outside


def test_argument_errors_come_before_any_library_call(monkeypatch):
    import nerf_replication_amd as pkg
    from nerf_replication_amd.occupancy import OccupancyGrid
    assert pkg.OccupancyGrid is OccupancyGrid
    monkeypatch.setattr(pkg._lib, "load", lambda: pytest.fail("argument errors must not reach the library"))
    net = pkg.Network()                                           # on the CPU: a GPU call would raise NerfLibraryError instead
    box = [-1, -1, -1, 1, 1, 1]
    with pytest.raises(TypeError):
        OccupancyGrid.from_network(object(), box, 8)
    for bad_box in ([0, 0, 0, 1, 1], [0, 0, 0, 1, 1, float("nan")], [0, 0, 0, 1, 1, -1], [0, 0, 0, 1, 1, 0], "box", None):
        with pytest.raises(ValueError):
            OccupancyGrid.from_network(net, bad_box, 8)
    for bad_n in (0, 1, -3, (4, 4), (4, 1, 4), 2.5, (2048, 2048, 512), "8"):
        with pytest.raises(ValueError):
            OccupancyGrid.from_network(net, box, bad_n)
    for bad_dilate in (-1, 1.5, True, "1", None):
        with pytest.raises(ValueError):
            OccupancyGrid.from_network(net, box, 8, dilate=bad_dilate)
    for bad_level in ("high", float("nan"), float("inf"), None, True):
        with pytest.raises(ValueError):
            OccupancyGrid.from_network(net, box, 8, level=bad_level)
    for bad_models in ((), ("medium",), ("fine", "fine"), 3, ("", "fine", "")):
        with pytest.raises(ValueError):
            OccupancyGrid.from_network(net, box, 8, models=bad_models)
    with pytest.raises(ValueError):
        OccupancyGrid.from_network(net, box, 8, chunk_lines=0)

    f = torch.zeros(4, 5, 6)
    with pytest.raises(ValueError):
        OccupancyGrid.from_fields(box)
    with pytest.raises(TypeError):
        OccupancyGrid.from_fields(box, fine=np.zeros((4, 5, 6), np.float32))
    with pytest.raises(ValueError):
        OccupancyGrid.from_fields(box, fine=f.double())
    with pytest.raises(ValueError):
        OccupancyGrid.from_fields(box, fine=f.permute(2, 1, 0))
    with pytest.raises(ValueError):
        OccupancyGrid.from_fields(box, coarse=f, fine=torch.zeros(4, 5, 7))
    with pytest.raises(ValueError):
        OccupancyGrid.from_fields(box, coarse=f, fine=torch.zeros(4, 5, 6, device="meta"))       # two devices
    with pytest.raises(ValueError):
        OccupancyGrid.from_fields(box, fine=torch.zeros(4, 1, 6))
    with pytest.raises(ValueError):
        OccupancyGrid.from_fields([0, 0, 0, 1, 0, 1], fine=f)
    with pytest.raises(ValueError):
        OccupancyGrid.from_fields(box, fine=f, dilate=-1)
    with pytest.raises(ValueError):
        OccupancyGrid.from_fields(box, fine=f, level=float("nan"))


def test_renderer_has_no_grid_by_default():
    import nerf_replication_amd as pkg
    r = pkg.Renderer(pkg.Network())
    assert r.occupancy is None and r.occupancy_stats is None


def test_lookup_frame_is_rounded_once():
    from nerf_replication_amd.occupancy import lookup_frame
    lo, inv = lookup_frame(np.array([[-2, -2, -2], [2, 2.5, 1]], np.float64), (64, 128, 3))
    assert lo.dtype == inv.dtype == np.float32
    assert np.array_equal(lo, np.float32([-2, -2, -2]))
    assert np.array_equal(inv, np.float32([63 / 4, 127 / 4.5, 2 / 3]))
    lo2, inv2 = O.lookup_frame([-2, -2, -2, 2, 2.5, 1], (64, 128, 3))
    assert np.array_equal(lo, lo2) and np.array_equal(inv, inv2)


def test_size_entries_refuse_without_a_gpu():
    """The size checks come first and touch neither a pointer nor the device."""
    import ctypes
    import nerf_replication_amd._lib as L
    lib = L.load()
    assert lib.nerf_occupancy_words(9, 12, 17) == 2 * ((8 * 11 * 16 + 63) // 64)
    assert lib.nerf_occupancy_words(33, 33, 33) == 1024 and lib.nerf_occupancy_words(2, 2, 2) == 2
    assert lib.nerf_occupancy_words(5, 5, 6) == 4                                        # 80 cells: 3 words, rounded up to 4
    assert lib.nerf_occupancy_words(1, 5, 5) == -1 and lib.nerf_occupancy_words(2048, 2048, 512) == -1
    assert lib.nerf_occupancy_build(None, 1, 4, 1, 4, 0.0, 0, None, None) == -1          # a dimension < 2
    assert lib.nerf_occupancy_build(None, 1, 2048, 2048, 512, 0.0, 0, None, None) == -1
    assert b"2^31" in lib.nerf_last_error()
    assert lib.nerf_occupancy_build(None, 1, 4, 4, 4, 0.0, -1, None, None) == -1         # negative dilate
    assert lib.nerf_occupancy_build(None, 0, 4, 4, 4, 0.0, 0, None, None) == -1          # stride < 1
    assert lib.nerf_occupancy_build(None, 1, 4, 4, 4, 0.0, 0, None, None) == -1          # null pointers
    i3, f3 = ctypes.c_int32 * 3, ctypes.c_float * 3
    ok = (i3(4, 4, 4), f3(-1, -1, -1), f3(1.5, 1.5, 1.5))
    assert lib.nerf_occupancy_mark(None, None, None, 0, 0, 64, None, *ok, 0, None, None) == 0          # no rays: a no-op
    assert lib.nerf_occupancy_mark(None, None, None, 0, 5, 64, None, *ok, 0, None, None) == -1         # null pointers
    assert lib.nerf_occupancy_mark(None, None, None, 0, 5, 64, None, i3(4, 1, 4), ok[1], ok[2], 0, None, None) == -1
    assert lib.nerf_occupancy_mark(None, None, None, 0, 5, 64, None, ok[0], ok[1], f3(1, 0, 1), 0, None, None) == -1
    assert lib.nerf_occupancy_mark(None, None, None, 0, 1 << 26, 64, None, *ok, 0, None, None) == -1   # 2^32 ids
    # the workspace: nerf_render_workspace_bytes' masked layout whatever fast_sampling is + the coarse mask and its list
    n = 640000
    assert lib.nerf_render_occupancy_workspace_bytes(n, 128, 0) == lib.nerf_render_occupancy_workspace_bytes(n, 128, 1) == \
        lib.nerf_render_workspace_bytes(n, 128, 1) + n * 64 + n * 256
    assert lib.nerf_render_occupancy_workspace_bytes(n, 0, 0) == lib.nerf_render_workspace_bytes(n, 0, 0) + n * 64 + n * 256
    assert lib.nerf_render_occupancy_workspace_bytes(-1, 128, 0) == -1
    # refusals of the render entry that need no device: fp16, and more rays than int32 point ids
    head = (None, None, None, None, 128, 1)           # packed_coarse .. white_bkgd
    rest = (0, 0.25, None, None, None, None, None, None, None, 0, None, None, None)      # fast_sampling .. stream
    assert lib.nerf_render_forward_occupancy(None, None, 8, *head, L.PREC_F16, *rest) == -4
    assert lib.nerf_render_forward_occupancy(None, None, 8, *head, L.PREC_F16S, *rest) == -4
    assert lib.nerf_render_forward_occupancy(None, None, 11184811, *head, L.PREC_F32, *rest) == -1
    assert lib.nerf_render_forward_occupancy(None, None, 0, *head, L.PREC_F32, *rest) == 0
