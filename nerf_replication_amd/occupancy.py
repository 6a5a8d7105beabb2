"""Occupancy grid: render without evaluating the samples that lie in empty space.

A bitfield over the cells of a density grid says where sigma can be positive; `Renderer.occupancy = grid` then sends only the
samples in occupied cells (or outside the box) through the networks and leaves raw = 0 at the others.  Compositing and the fine
sampler both apply relu(sigma), so the image is bit-equal to the plain render wherever every culled sample has a true sigma <= 0:
exact wherever the grid is right, and the grid is made conservative by dilation.  The density comes from density_grid (the
fused MLP kernels), the bitfield and the lookup from the nerf_occupancy_* kernels (include/nerf_mi355x.h has the definitions);
torch only moves tensors.  No CPU fallback.

Training: `Renderer.train_occupancy = grid` culls the fine pass of the training step with the fine bitfield
(the coarse one is ignored there), and OccupancyGrid.refresh rebuilds a bitfield in place from the network as it is now; `hold`
keeps a grid point occupied for that many refreshes after it was last above the level (nerf_occupancy_age).
"""
import ctypes
import numbers

import numpy as np
import torch

from . import _lib
from .mesh import _bbox, _field_layout, _shape3, density_grid
from .network import Network

MODELS = ("", "fine")


def _grid_frame(bbox, N):
    """(bbox [2,3] float64, dims) of an occupancy grid: every size >= 2 and every axis extent > 0."""
    dims, b = _shape3(N), _bbox(bbox)
    if min(dims) < 2:
        raise ValueError(f"an occupancy grid needs at least 2 points per axis, got {dims}")
    if (b[1] <= b[0]).any():
        raise ValueError(f"bbox must have a positive extent on every axis, got {bbox!r}")
    return b, dims


def _level(level):
    if isinstance(level, bool) or not isinstance(level, numbers.Real) or not np.isfinite(level):
        raise ValueError(f"level must be a finite number, got {level!r}")
    return float(level)


def _dilate(dilate):
    if isinstance(dilate, bool) or not isinstance(dilate, numbers.Integral) or dilate < 0 or dilate > 2 ** 31 - 1:
        raise ValueError(f"dilate must be an int >= 0 (cells), got {dilate!r}")
    return int(dilate)


def lookup_frame(bbox, dims):
    """(box_min, inv_step) of the sample lookup: fp32(min) and fp32((n - 1) / (max - min)), computed in float64, rounded once."""
    b = np.asarray(bbox, dtype=np.float64).reshape(2, 3)
    inv = (np.asarray(dims, dtype=np.float64) - 1.0) / (b[1] - b[0])
    return b[0].astype(np.float32), inv.astype(np.float32)


def _hold(hold):
    if isinstance(hold, bool) or not isinstance(hold, numbers.Integral) or hold < 1 or hold > 255:
        raise ValueError(f"hold must be an int in [1, 255] (refreshes), got {hold!r}")
    return int(hold)


def _params_key(net, model):
    sub = net.model_fine if model == "fine" else net.model
    return tuple((p.data_ptr(), p._version) for p in sub.ordered_params())


class OccupancyGrid:
    """One bitfield per model ("" coarse, "fine") over the (nx-1)(ny-1)(nz-1) cells of a grid on `bbox`.

    The coarse bitfield culls the 64 coarse samples, the fine one the 192 merged samples (with N_importance = 0 the coarse
    network draws the frame and only the coarse bitfield is used).  A missing bitfield means that pass runs on every sample.
    Build with from_network or from_fields.

    refresh(net) rebuilds bitfields in place from `net` as it is now.  `hold` (int in [1, 255], default 1, read by refresh): a grid
    point counts as occupied if it was above the level in one of the last `hold` refreshes.  It looks back over refreshes only: the
    build that created the grid is not remembered.  `uses` counts the training steps served since the last refresh
    (Renderer.train_occupancy)."""

    def __init__(self, bbox, dims, level, dilate, bits, keys, chunk_lines=None):
        self.bbox, self.dims, self.level, self.dilate = bbox, dims, level, dilate
        self.chunk_lines = chunk_lines        # density_grid's chunking, as from_network was given it
        self.hold, self.uses = 1, 0
        self._age = {}                        # model -> uint8 [nx*ny*nz]: refreshes since the point was last above the level
        self.bits = bits                      # model -> int32 [words] device tensor, or None
        self.keys = keys                      # model -> parameter key at build time; None: built from fields, never stale
        self.box_min, self.inv_step = lookup_frame(bbox, dims)
        self.device = next(b.device for b in bits.values() if b is not None)

    @classmethod
    def from_network(cls, net, bbox, N=128, level=0.0, dilate=1, models=MODELS, chunk_lines=None):
        """The grid of `net` as it is now: one density_grid per model in `models`, then the bitfield.  Records the
        (data_ptr, _version) of the parameters, as Network.packed does: Renderer.render refuses the grid once they changed."""
        if not isinstance(net, Network):
            raise TypeError("OccupancyGrid.from_network needs a nerf_replication_amd Network")
        b, dims = _grid_frame(bbox, N)
        level, dilate = _level(level), _dilate(dilate)
        try:
            models = tuple(models)
        except TypeError:
            raise ValueError(f'models must be a sequence out of ("", "fine"), got {models!r}') from None
        if not models or len(set(models)) != len(models) or any(m not in MODELS for m in models):
            raise ValueError(f'models must be a non-empty sequence out of ("", "fine") without repeats, got {models!r}')
        if chunk_lines is not None and (not isinstance(chunk_lines, numbers.Integral) or chunk_lines < 1):
            raise ValueError(f"chunk_lines must be a positive int, got {chunk_lines!r}")
        bits, keys = {m: None for m in MODELS}, {}
        for m in models:
            keys[m] = _params_key(net, m)
            bits[m] = _build(density_grid(net, b.reshape(-1), dims, model=m, chunk_lines=chunk_lines), level, dilate)
        return cls(b, dims, level, dilate, bits, keys, chunk_lines)

    @classmethod
    def from_fields(cls, bbox, coarse=None, fine=None, level=0.0, dilate=1):
        """The grid of any [nx,ny,nz] device fields (or raw [nx,ny,nz,4] buffers), e.g. what density_grid / extract_mesh already
        produced: `coarse` culls the coarse pass, `fine` the fine pass.  No parameter key is recorded, so there is NO staleness
        check: the caller keeps the fields in step with the network.  Passing the fine model's field as `coarse` is allowed but
        lossy: the two models differ, and a coarse sample culled where the coarse sigma is positive moves the fine samples."""
        if coarse is None and fine is None:
            raise ValueError("from_fields needs a coarse or a fine field")
        layouts = {m: _field_layout(f) for m, f in (("", coarse), ("fine", fine)) if f is not None}
        shapes = {lay[2] for lay in layouts.values()}
        if len(shapes) != 1:
            raise ValueError(f"the coarse and the fine field must have one shape, got {sorted(shapes)}")
        if len({lay[0].device for lay in layouts.values()}) != 1:
            raise ValueError("the coarse and the fine field must be on one device")
        b, dims = _grid_frame(bbox, shapes.pop())
        level, dilate = _level(level), _dilate(dilate)
        bits = {m: None for m in MODELS}
        for m, (field, _, _) in layouts.items():
            bits[m] = _build(field, level, dilate)
        return cls(b, dims, level, dilate, bits, None)

    def _bits(self, model):
        if model not in MODELS:
            raise ValueError(f'model must be "" (coarse) or "fine", got {model!r}')
        if self.bits[model] is None:
            raise ValueError(f"this grid has no bitfield for model {model!r}")
        return self.bits[model]

    def cells(self, model="fine"):
        """The unpacked bits: bool [nx-1, ny-1, nz-1] on the device (for tests and inspection)."""
        words = self._bits(model)
        cx, cy, cz = (n - 1 for n in self.dims)
        shifts = torch.arange(32, dtype=torch.int32, device=words.device)
        return ((words[:, None] >> shifts) & 1).reshape(-1)[:cx * cy * cz].bool().view(cx, cy, cz)

    def occupied_fraction(self, model="fine"):
        return float(self.cells(model).float().mean().item())

    def stale(self, net, model):
        """True iff the grid was built from a network whose `model` parameters have since changed (or from another network)."""
        return self.keys is not None and model in self.keys and self.keys[model] != _params_key(net, model)

    def refresh(self, net, models=None):
        """Rebuild the bitfields of `models` (default: those the grid has) IN PLACE from `net` as it is now, in its current
        precision and under no_grad: density_grid on the grid's bbox and dims, nerf_occupancy_age with self.hold, nerf_occupancy_build
        into the existing words (same data_ptr, same word count).  Afterwards the key of each model is the network's current one
        (stale() is False) and uses = 0.  The age state, one uint8 per grid point and model, is created (255 everywhere) at a model's
        first refresh, so `hold` looks back over refreshes only, not to the build that created the grid.  A grid from from_fields can be
        refreshed too; it then carries a key."""
        hold = _hold(self.hold)
        if not isinstance(net, Network):
            raise TypeError("OccupancyGrid.refresh needs a nerf_replication_amd Network")
        if models is None:
            models = tuple(m for m in MODELS if self.bits[m] is not None)
        try:
            models = tuple(models)
        except TypeError:
            raise ValueError(f'models must be a sequence out of ("", "fine"), got {models!r}') from None
        if not models or len(set(models)) != len(models):
            raise ValueError(f'models must be a non-empty sequence out of ("", "fine") without repeats, got {models!r}')
        for m in models:
            self._bits(m)
        nx, ny, nz = self.dims
        with torch.no_grad():
            for m in models:
                bits, key = self.bits[m], _params_key(net, m)
                field = density_grid(net, self.bbox.reshape(-1), self.dims, model=m, chunk_lines=self.chunk_lines)
                if field.device != self.device:
                    raise ValueError(f"the occupancy grid is on {self.device}, the network on {field.device}")
                if int(_lib.call("nerf_occupancy_words", nx, ny, nz)) != bits.numel():
                    raise _lib.NerfLibraryError(f"the bitfield of model {m!r} does not have the words of a {self.dims} grid")
                age = self._age.get(m)
                if age is None:
                    age = self._age[m] = torch.full((field.numel(),), 255, dtype=torch.uint8, device=self.device)
                # `on` overwrites the field: it is not needed again
                _lib.call("nerf_occupancy_age", field, 1, field.numel(), self.level, hold, age, field)
                _lib.call("nerf_occupancy_build", field, 1, nx, ny, nz, 0.0, self.dilate, bits)
                if self.keys is None:
                    self.keys = {}
                self.keys[m] = key
        self.uses = 0

    def lookup_args(self):
        """(dims, box_min, inv_step) as the HOST arrays of nerf_occupancy_mark / nerf_render_forward_occupancy."""
        return ((ctypes.c_int32 * 3)(*self.dims), (ctypes.c_float * 3)(*self.box_min.tolist()),
                (ctypes.c_float * 3)(*self.inv_step.tolist()))


def _build(field, level, dilate):
    """nerf_occupancy_build of one field -> int32 [words]."""
    field, stride, (nx, ny, nz) = _field_layout(field)
    if not field.is_cuda:
        raise _lib.NerfLibraryError("an occupancy grid needs its field on a GPU (cuda) device; there is no CPU fallback")
    n_words = int(_lib.call("nerf_occupancy_words", nx, ny, nz))
    if n_words < 0:
        raise _lib.NerfLibraryError(f"nerf_occupancy_words refused a grid of {nx} x {ny} x {nz} points")
    bits = torch.empty(n_words, dtype=torch.int32, device=field.device)
    _lib.call("nerf_occupancy_build", _lib.strided(field), stride, nx, ny, nz, level, dilate, bits)     # layout: _field_layout
    return bits
