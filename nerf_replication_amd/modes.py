"""Which path a call of the renderer takes, and what it refuses: the facts of one call, one ordered table, one resolver.

Renderer.render, Renderer.render_geometry and training.render_with_grad gather a Facts record, call resolve() and dispatch on the
name it returns.  TABLE is walked from the top, group by group and row by row: the first row whose predicate holds decides -- an exception with its message, a
check of a value that stays a function (the grid objects, geometry_block_rays), or the name of a path.  The order of the rows IS the
precedence of the refusals, and the position of the "empty" rows is where an empty batch returns among them.  Nothing here touches a
tensor, a device or the library: the rows that look at a grid are skipped when no renderer is given, so resolve(facts) runs anywhere.

The paths: frame / frame_stochastic / frame_occupancy (nerf_render_forward and its _stochastic / _occupancy siblings), step /
step_masked / step_coarse / step_culled (training.RenderFunction / Masked- / Coarse- / CulledRenderFunction), geometry (the staged
pass of render_geometry), empty (a batch without rays: no launch).
"""
from typing import NamedTuple

import torch

from . import _lib

RENDER, GEOMETRY, STEP = "render", "render_geometry", "render_with_grad"


def precision_of(net):
    return getattr(net, "precision", "f32")


class Facts(NamedTuple):
    """What one call depends on, read from the renderer once, at call time."""
    call: str                   # RENDER, GEOMETRY or STEP
    precision: str              # the network's precision name
    task: str
    perturb: bool
    fast_sampling: bool
    N_importance: int
    occupancy: bool             # Renderer.occupancy is set
    train_occupancy: bool       # Renderer.train_occupancy is set (STEP: a grid was handed over)
    rays_grad: bool             # the rays require grad (RENDER: and autograd is on)
    with_grad: bool             # a training call, or rays_grad
    empty: bool                 # n == 0
    draws: bool                 # the call carries random draws: a jitter, a per-ray u, or both

    @property
    def fp32(self):
        return _lib.fp32_accurate(self.precision)

    @property
    def stochastic(self):
        return self.perturb or self.task == "train"


def facts(renderer, call, rays_grad, n, draws=None, train_occupancy=None):
    """The Facts of `call` on `renderer`.  STEP (render_with_grad) passes what it was handed: `draws`, `train_occupancy`."""
    net, task, perturb, n_imp = renderer.net, renderer.task, bool(renderer.perturb), renderer.N_importance
    with_grad = bool(rays_grad) or call == STEP or (torch.is_grad_enabled() and getattr(net, "training", False) and
                                                    any(p.requires_grad for p in net.parameters()))
    return Facts(call, precision_of(net), task, perturb, bool(renderer.fast_sampling), n_imp, renderer.occupancy is not None,
                 renderer.train_occupancy is not None if train_occupancy is None else train_occupancy, bool(rays_grad), with_grad,
                 n == 0, perturb or (task == "train" and n_imp > 0) if draws is None else draws)


# ---- the checks that stay functions: values of objects, not modes.  (renderer, dev) -> None, or raise
def _grid_type():
    from .occupancy import OccupancyGrid
    return OccupancyGrid


def _occupancy_is_a_grid(renderer, dev):
    if not isinstance(renderer.occupancy, _grid_type()):
        raise TypeError("Renderer.occupancy must be an OccupancyGrid or None")


def _occupancy_grid_usable(renderer, dev):
    grid = renderer.occupancy
    if grid.device != dev:
        raise ValueError(f"the occupancy grid is on {grid.device}, the rays on {dev}")
    for model in ("", "fine") if renderer.N_importance > 0 else ("",):
        if grid.stale(renderer.net, model):
            raise RuntimeError("the network's parameters changed since the occupancy grid was built from them: rebuild the "
                               "grid (OccupancyGrid.from_network), or set Renderer.occupancy = None")


def _train_grid_usable(renderer, dev):
    grid, every = renderer.train_occupancy, renderer.train_occupancy_every
    if not isinstance(grid, _grid_type()):
        raise TypeError("Renderer.train_occupancy must be an OccupancyGrid or None")
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError(f"Renderer.train_occupancy_every must be an int >= 1 (steps), got {every!r}")
    if grid.bits["fine"] is None:
        raise ValueError("Renderer.train_occupancy needs a grid with a fine bitfield: the training step culls the fine pass only")
    if grid.device != dev:
        raise ValueError(f"the occupancy grid is on {grid.device}, the rays on {dev}")


def _geometry_block_rays(renderer, dev):
    block = renderer.geometry_block_rays
    if isinstance(block, bool) or not isinstance(block, int) or block < 1:
        raise ValueError(f"Renderer.geometry_block_rays must be an int >= 1 (rays), got {block!r}")


# ---- the table: groups of rows, (when the group applies, its rows).  A row is (predicate over Facts, outcome); an outcome is
# (exception type, message template over f = the facts), one of the functions above, or the name of a path
NIE = NotImplementedError
_MODE = "(task={f.task!r}, perturb={f.perturb})"


def _always(f):
    return True


# the modes without adjoint kernels: fp16 precisions, and gradients with respect to the rays with fast_sampling or
# N_importance == 0 -- those two modes train their parameters only.  The precision row tests the NAMES: the alias "fp32" is refused
DIFFERENTIABLE = (
    (lambda f: f.precision not in ("f32", "f32x"),
     (NIE, "training runs on the fp32-accurate paths: precision 'f32' (exact fp32 MFMA) or 'f32x' "
           "(forward on split-fp16 MFMA; the backward kernels are fp32 MFMA either way)")),
    (lambda f: f.N_importance not in (0, _lib.N_IMPORTANCE),
     (NIE, "training path is built for N_importance in {{0, 128}}")),
    (lambda f: f.rays_grad and (f.N_importance != _lib.N_IMPORTANCE or f.fast_sampling),
     (NIE, "gradients with respect to the rays are built for N_importance=128 without fast_sampling")),
)
CHECK_DIFFERENTIABLE = ((_always, DIFFERENTIABLE),)          # training.check_differentiable: that block alone

TABLE = (
    # ---- Renderer.render.  Rays that require grad first: never a detached result for them
    (lambda f: f.call == RENDER and f.rays_grad, DIFFERENTIABLE),
    # Renderer.occupancy set
    (lambda f: f.call == RENDER and f.occupancy, (
        (_always, _occupancy_is_a_grid),
        (lambda f: f.with_grad,
         (NIE, "occupancy culling is an inference feature: no training step and no ray gradients with Renderer.occupancy set")),
        (lambda f: f.stochastic,
         (NIE, "occupancy culling is not built for stochastic sampling " + _MODE)),
        (lambda f: not f.fp32,
         (NIE, "occupancy culling runs in precision 'f32' or 'f32x', not {f.precision!r}: the fp16 far-plane "
               "guard is not defined on a culled list")),
        (_always, _occupancy_grid_usable),
    )),
    # stochastic sampling
    (lambda f: f.call == RENDER and f.stochastic, (
        (lambda f: not f.fp32,
         (NIE, "stochastic sampling " + _MODE + " runs in precision 'f32' or 'f32x', not {f.precision!r}")),
        (lambda f: f.fast_sampling,
         (NIE, "stochastic sampling " + _MODE + " is not built with fast_sampling")),
    )),
    # a training call with Renderer.train_occupancy set; under no_grad / eval() the attribute is not looked at
    (lambda f: f.call == RENDER and f.with_grad and f.train_occupancy, (
        *DIFFERENTIABLE,
        (_always, _train_grid_usable),
        (lambda f: f.rays_grad,
         (NIE, "no ray gradients with Renderer.train_occupancy set: the masked backward forms no point gradients")),
        (lambda f: f.N_importance == 0,
         (NIE, "Renderer.train_occupancy culls the fine pass: there is none with N_importance = 0")),
    )),
    # an empty batch under autograd returns here: after the rows above, before the step's own
    (lambda f: f.call == RENDER and f.with_grad and f.empty, ((_always, "empty"),)),
    # ---- the step: training.render_with_grad, and Renderer.render on its way there
    (lambda f: f.call == STEP or (f.call == RENDER and f.with_grad), (
        *DIFFERENTIABLE,
        (lambda f: f.train_occupancy and (f.rays_grad or f.N_importance != _lib.N_IMPORTANCE or (f.draws and f.fast_sampling)),
         (NIE, "the culled step trains parameters with N_importance=128; fast_sampling with deterministic sampling only")),
        (lambda f: not f.train_occupancy and (f.N_importance == 0 or f.fast_sampling) and f.draws,
         (NIE, "stochastic sampling trains with N_importance=128 without fast_sampling only")),
        (lambda f: f.train_occupancy, "step_culled"),
        (lambda f: f.N_importance == 0, "step_coarse"),
        (lambda f: f.fast_sampling, "step_masked"),
        (_always, "step"),
    )),
    # ---- Renderer.render, inference: the whole-frame entries.  An empty batch returns after every refusal
    (lambda f: f.call == RENDER, (
        (lambda f: f.empty, "empty"),
        (lambda f: f.stochastic, "frame_stochastic"),
        (lambda f: f.occupancy, "frame_occupancy"),
        (_always, "frame"),
    )),
    # ---- Renderer.render_geometry: each refusal names the mode
    (lambda f: f.call == GEOMETRY, (
        (lambda f: f.rays_grad,
         (NIE, "render_geometry has no autograd path: rays that require grad are refused (detach them; "
               "render() is the differentiable call)")),
        (lambda f: not f.fp32,
         (NIE, "render_geometry runs in precision 'f32' or 'f32x', not {f.precision!r}: the gradient chain has no fp16 form")),
        (lambda f: f.fast_sampling,
         (NIE, "render_geometry is not built with fast_sampling")),
        (lambda f: f.occupancy,
         (NIE, "render_geometry is not built with occupancy culling: set Renderer.occupancy = None")),
        (lambda f: f.stochastic,
         (NIE, "render_geometry is not built for stochastic sampling " + _MODE)),
        (_always, _geometry_block_rays),
        (lambda f: f.empty, "empty"),
        (_always, "geometry"),
    )),
)


def resolve(f, renderer=None, dev=None, table=TABLE):
    """Walk `table` with the facts `f`: raise at the first refusal that applies, return the first path.  `renderer` and `dev` (the
    rays' device) are what the value checks look at; without a renderer they are passed over."""
    for applies, rows in table:
        if not applies(f):
            continue
        for predicate, outcome in rows:
            if not predicate(f):
                continue
            if isinstance(outcome, str):
                return outcome
            if isinstance(outcome, tuple):
                raise outcome[0](outcome[1].format(f=f))
            if renderer is not None:
                outcome(renderer, dev)
    return None
