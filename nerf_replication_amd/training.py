"""Training path (BASELINE config 3): Renderer.render under autograd, fp32.

The reference trains by calling the same Renderer.render with autograd on (src/train/trainers/nerf.py:27,
trainer.py:53-60): MSE on the fine RGB only, and -- because fine_sample_points does not detach the
coarse weights -- the coarse network learns through the sample positions.  Here the
forward runs the SAVE-mode fused kernels and the backward is the chain of adjoint kernels behind the
C ABI (nerf_composite_backward, nerf_mlp_backward, nerf_sample_fine_backward); torch.autograd only
carries the 48 parameter gradients back to the optimizer.  No ATen op computes on this path.

The rays are differentiable inputs too (camera-pose refinement, iNeRF-style pose estimation): when rays_o / rays_d require grad,
both MLP chains also emit the point gradients (nerf_mlp_backward_rays_x) and nerf_rays_viewdirs_backward / nerf_rays_backward
reduce them per ray.  Parameters that do not require grad get None; with none at all the chains run alone (no weight-gradient
launch).  A step whose rays do not require grad runs exactly the launches it ran before.

In the reference's training sampling mode (Renderer.task == "train") the step takes the two draws of Renderer._draws: the
jittered coarse depths (nerf_stratified_samples) go to the coarse forward / backward and the sampler with a per-ray stride of
64, the per-ray u to the sampler and its adjoint with a stride of 128.  Without draws every launch is the deterministic one.

Two more modes train, with deterministic sampling and parameter gradients: fast_sampling (MaskedRenderFunction: the reference's
ESS / ERT mask, volume_renderer.py:132-244 / :359-369 / network.py:207-253 -- the fine network, its activation store and its
backward run on the valid merged samples only, compacted on the device) and N_importance == 0 (CoarseRenderFunction: the coarse
network alone, composited over its 64 samples).  The unmasked step above issues exactly the launches it issued before.

With Renderer.train_occupancy set (CulledRenderFunction) the fine pass runs on the merged samples the grid's fine
bitfield keeps, deterministic or stochastic, through the same masked entries; with fast_sampling the list is the sampler's mask AND
the lookup.  Compositing's adjoint is exactly zero wherever sigma <= 0, so the step has the plain step's gradients wherever the
grid is right.
"""
import torch

from . import _lib, modes


class _Step:
    """The stages of a training step.  Each stage owns the buffers it fills and knows the C entry that fills them; the autograd
    functions below order the stages and carry tensors from forward to backward.  All of it is enqueued on the current stream."""

    S_c, S_f = _lib.N_SAMPLES, _lib.N_SAMPLES + _lib.N_IMPORTANCE

    def __init__(self, renderer, rays_o, rays_d, prec=None, stochastic=None):
        self.renderer, self.rays_o, self.rays_d = renderer, rays_o, rays_d
        self.dev, self.n = rays_o.device, rays_o.shape[0]
        self.prec = _lib.PRECISIONS[modes.precision_of(renderer.net)] if prec is None else prec
        self.white = int(bool(renderer.white_bkgd))
        # the coarse depths and u with their per-ray strides (0: the shared tables)
        self.t_c, self.u = renderer._get_tables(self.dev)
        self.t_cs, self.u_s = 0, 0
        if stochastic is not None:
            self.t_c, self.t_cs, self.u, self.u_s = stochastic
        self.pk_b = self.gsave = None

    def empty(self, *shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.dev)

    def _rays(self, tvals, stride, S):
        return self.rays_o, self.rays_d, tvals, stride, self.n, S

    # ---- forward stages
    def use_draws(self, jitter, u_rays):
        """The reference's training-mode draws: jittered coarse depths [n,64] and / or a per-ray u [n,128]."""
        if jitter is not None:
            t_lin, self.t_c, self.t_cs = self.t_c, self.empty(self.n, self.S_c), self.S_c
            _lib.call("nerf_stratified_samples", t_lin, jitter, self.n, self.t_c)
        if u_rays is not None:
            self.u, self.u_s = u_rays, _lib.N_IMPORTANCE
        return self.t_c, self.t_cs, self.u, self.u_s

    def forward_save(self, packed, tvals, stride, S, density_only=False, masked=None, raw=None):
        """SAVE forward of the packed model over S samples per ray -> (raw [n,S,4], save).  density_only: the sigma head alone.
        Otherwise raw goes to compositing only and its gradient will come from compositing's adjoint (zero wherever sigma <= 0):
        tiles without density skip the colour branch and its stores (exact, see the header).  masked = (index, count): the compact
        rows of those samples alone; the others keep what `raw` holds."""
        raw = self.empty(self.n, S, 4) if raw is None else raw
        save = self.empty(int(_lib.call("nerf_train_save_floats", self.n * S)))
        tail = (packed, raw, save, self.prec)
        if masked is not None:
            _lib.call("nerf_mlp_forward_rays_save_masked", *self._rays(tvals, stride, S), *masked, *tail)
        elif density_only:
            _lib.call("nerf_mlp_forward_rays_save_density", *self._rays(tvals, stride, S), *tail)
        else:
            _lib.call("nerf_mlp_forward_rays_save_for_compositing", *self._rays(tvals, stride, S), *tail)
        return raw, save

    def sample_fine(self, raw_c, fast_sampling=False):
        """Coarse sigma -> the 192 merged depths t_sorted [n,192]; fast_sampling: and their validity (ESS / ERT) as uint8."""
        t_sorted = self.empty(self.n, self.S_f)
        valid = self.empty(self.n, self.S_f, dtype=torch.uint8) if fast_sampling else None
        thresholds = (float(self.renderer.weights_threshold), 0.45) if fast_sampling else (0.0, 0.0)
        _lib.call("nerf_sample_fine_rays", raw_c, self.t_c, self.t_cs, self.u, self.u_s, self.n, t_sorted, None, valid, *thresholds)
        return t_sorted, valid

    def mark(self, grid, tvals, S, valid=None):
        """The grid's fine bitfield looked up at the S depths of every ray -> valid [n,S] uint8; ANDed into `valid` if given."""
        out = self.empty(self.n, S, dtype=torch.uint8) if valid is None else valid
        _lib.call("nerf_occupancy_mark", *self._rays(tvals, S, S), grid.bits["fine"], *grid.lookup_args(), int(valid is not None), out)
        return out

    def compact(self, valid):
        """-> (ids of the valid samples, their number), both on the device."""
        P = valid.numel()
        index, count = self.empty(P, dtype=torch.int32), self.empty(1, dtype=torch.int32)
        ws = self.empty(int(_lib.call("nerf_compact_valid_workspace_bytes", P)), dtype=torch.uint8)
        _lib.call("nerf_compact_valid", valid, P, index, count, ws)
        return index, count

    def composite(self, raw, tvals, stride, S):
        rgb, depth = self.empty(self.n, 3), self.empty(self.n)
        _lib.call("nerf_composite", raw, tvals, stride, self.n, S, self.white, rgb, depth, None)
        return rgb, depth

    # ---- backward stages
    def begin_backward(self, ctx, g_rgb, g_depth, n_inputs):
        """The incoming gradients as contiguous fp32, and one gradient tensor per parameter (inputs from `n_inputs` on) as views
        of one zeroed buffer; no buffer when no parameter needs grad."""
        self.g_rgb = g_rgb.contiguous().to(torch.float32)
        self.g_depth = None if g_depth is None else g_depth.contiguous().to(torch.float32)
        self.params, self.need_params = ctx.params, ctx.needs_input_grad[n_inputs:]
        self.grads = _lib.zeroed_grads(self.params, self.dev) if any(self.need_params) else None

    def param_grads(self):
        return tuple(g.to(p.dtype) if need else None
                     for g, p, need in zip(self.grads or [None] * len(self.params), self.params, self.need_params))

    def composite_backward(self, raw, tvals, stride, S, depths=True):
        """image -> (g_raw [n,S,4], g_t [n,S] | None: the depths are constants)"""
        g_raw = self.empty(self.n, S, 4)
        g_t = self.empty(self.n, S) if depths else None
        _lib.call("nerf_composite_backward", raw, tvals, stride, self.n, S, self.white, self.g_rgb, self.g_depth, g_raw, g_t)
        return g_raw, g_t

    def _pack_bwd(self, params):
        if self.pk_b is None:
            self.pk_b = self.empty(int(_lib.call("nerf_packed_bwd_bytes", self.prec)), dtype=torch.uint8)
        _lib.call("nerf_pack_model_bwd", [p.detach().contiguous() for p in params], self.pk_b, self.prec)
        return self.pk_b

    def _gsave(self, S):
        """The chain's buffer: allocated by the first (fine) pass, its head reused by the coarse one."""
        floats = int(_lib.call("nerf_train_grad_floats", self.n * S))
        if self.gsave is None:
            self.gsave = self.empty(floats)
        return self.gsave[:floats]

    def live_count(self, S):
        """For the renderer.live_tile_stats hook: the live-tile count the backward over S samples left in gsave, as a 1-element
        device tensor (no host sync here).  A clone: the next pass reuses gsave."""
        if getattr(self.renderer, "live_tile_stats", None) is None:
            return None
        return self._gsave(S)[int(_lib.call("nerf_train_live_count_offset", self.n * S))].view(torch.int32).clone()

    def mlp_backward(self, params, grads, tvals, stride, S, g_raw, save, density_only=False, depths=True, points=False):
        """g_raw -> the gradients of `params` accumulated into `grads` (None: no parameter needs grad, the chain runs alone),
        g_t [n,S] of the sample points (if `depths`) and g_x [n,S,3] (if `points`: the rays require grad)."""
        pk_b = self._pack_bwd(params)
        g_t = self.empty(self.n, S) if depths else None
        g_x = self.empty(self.n, S, 3) if points else None
        head = self._rays(tvals, stride, S) + (pk_b, g_raw, save, self._gsave(S), g_t)
        if points:
            _lib.call("nerf_mlp_backward_rays_x", *head, g_x, grads, int(density_only), self.prec)
        elif density_only:
            _lib.call("nerf_mlp_backward_density", *head, grads, self.prec)
        else:
            _lib.call("nerf_mlp_backward", *head, grads, self.prec)
        return g_t, g_x

    def mlp_backward_masked(self, params, grads, tvals, S, masked, g_raw, save):
        """The MLP backward over the compact rows of the valid samples -> their g_t scattered back, 0 at the masked ones."""
        pk_b = self._pack_bwd(params)
        g_t = self.empty(self.n, S)
        ws = self.empty(int(_lib.call("nerf_mlp_backward_masked_workspace_bytes", self.n * S)), dtype=torch.uint8)
        _lib.call("nerf_mlp_backward_masked", *self._rays(tvals, S, S), *masked, pk_b, g_raw, save, self._gsave(S), g_t, grads, self.prec, ws)
        return g_t

    def coarse_backward(self, raw_c, save_c, t_sorted, g_t, cnt_f, ray_terms=None):
        """The coarse pass of a hierarchical step: depths -> coarse density -> coarse MLP parameters.  ray_terms = (g_x_fine,
        g_dview) when the rays require grad: -> (g_rays_o, g_rays_d)."""
        g_raw_c = self.empty(self.n, self.S_c, 4)
        _lib.call("nerf_sample_fine_rays_backward", raw_c, self.t_c, self.t_cs, self.u, self.u_s, self.n, t_sorted, g_t, g_raw_c)
        cap = getattr(self.renderer, "capture_adjoints", None)
        if cap is not None:       # tests: the per-ray sampler adjoint d loss / d raw_coarse and d loss / d t_sorted (parity attribution)
            cap["g_raw_coarse"], cap["g_t_sorted"], cap["raw_coarse"] = g_raw_c.clone(), g_t.clone(), raw_c.clone()
            cap["t_sorted"] = t_sorted.clone()
        # only the coarse sigma was ever used: the density-only backward
        _, g_x_c = self.mlp_backward(self.params[:24], None if self.grads is None else self.grads[:24], self.t_c, self.t_cs, self.S_c,
                                     g_raw_c, save_c, density_only=True, depths=False, points=ray_terms is not None)
        g_rays = None
        if ray_terms is not None:
            g_rays = self.empty(self.n, 3), self.empty(self.n, 3)
            _lib.call("nerf_rays_backward", self.n, self.t_c, self.t_cs, g_x_c, t_sorted, *ray_terms, *g_rays)
        stats = getattr(self.renderer, "live_tile_stats", None)
        if stats is not None:     # (live tiles, tiles) of the fine and of the coarse pass
            stats.append((cnt_f, self.n * self.S_f // 32, self.live_count(self.S_c), self.n * self.S_c // 32))
        return g_rays


class RenderFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, renderer, rays_o, rays_d, draws, *params):
        s = _Step(renderer, rays_o, rays_d)
        ctx.stochastic = s.use_draws(*draws) if draws is not None else None
        pk_c, pk_f = renderer.net.packed(""), renderer.net.packed("fine")
        # coarse pass: only its sigma is ever used (it places the fine samples; the coarse colour is never
        # composited) -> the density-only forward / backward pair
        raw_c, save_c = s.forward_save(pk_c, s.t_c, s.t_cs, s.S_c, density_only=True)
        t_sorted, _ = s.sample_fine(raw_c)
        raw_f, save_f = s.forward_save(pk_f, t_sorted, s.S_f, s.S_f)
        rgb, depth = s.composite(raw_f, t_sorted, s.S_f, s.S_f)
        ctx.renderer, ctx.prec, ctx.params = renderer, s.prec, params
        ctx.save_for_backward(rays_o, rays_d, raw_c, save_c, t_sorted, raw_f, save_f)
        return rgb, depth

    @staticmethod
    def backward(ctx, g_rgb, g_depth):
        rays_o, rays_d, raw_c, save_c, t_sorted, raw_f, save_f = ctx.saved_tensors
        s = _Step(ctx.renderer, rays_o, rays_d, ctx.prec, ctx.stochastic)
        need_rays = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        s.begin_backward(ctx, g_rgb, g_depth, 4)
        # fine pass: image -> raw_fine and depths; MLP backward; points -> depths
        g_raw_f, g_t = s.composite_backward(raw_f, t_sorted, s.S_f, s.S_f)
        g_t_pts, g_x_f = s.mlp_backward(s.params[24:], None if s.grads is None else s.grads[24:], t_sorted, s.S_f, s.S_f,
                                        g_raw_f, save_f, points=need_rays)
        ray_terms = None
        if need_rays:
            # the view-direction term reads the fine g_zv rows: before the coarse pass reuses gsave
            g_dview = s.empty(s.n, 3)
            w_views = s.params[24 + 16].detach().contiguous()           # model_fine views_linears.0.weight [128,283]
            _lib.call("nerf_rays_viewdirs_backward", rays_d, s.n, s.S_f, s.gsave, w_views, g_dview)
            ray_terms = (g_x_f, g_dview)
        g_t.add_(g_t_pts)                     # plumbing: one elementwise add of two [n,192] buffers
        g_rays = s.coarse_backward(raw_c, save_c, t_sorted, g_t, s.live_count(s.S_f), ray_terms)
        g_rays = (g_rays[0] if need_rays and ctx.needs_input_grad[1] else None, g_rays[1] if need_rays and ctx.needs_input_grad[2] else None)
        return (None,) + g_rays + (None,) + s.param_grads()


def _masked_forward(ctx, renderer, rays_o, rays_d, draws, grid, params):
    """The forward of a step whose fine pass runs on a compact list: the sampler's mask (fast_sampling), the lookup of `grid`'s fine
    bitfield at the merged depths, or both ANDed.  The coarse pass is the plain step's, on the shared or the drawn depths."""
    s = _Step(renderer, rays_o, rays_d)
    pk_c, pk_f = renderer.net.packed(""), renderer.net.packed("fine")
    raw_f = torch.zeros((s.n, s.S_f, 4), dtype=torch.float32, device=s.dev)           # unlisted samples keep raw = 0
    ctx.stochastic = s.use_draws(*draws) if draws is not None else None
    raw_c, save_c = s.forward_save(pk_c, s.t_c, s.t_cs, s.S_c, density_only=True)
    t_sorted, valid = s.sample_fine(raw_c, fast_sampling=grid is None or bool(renderer.fast_sampling))
    if grid is not None:
        valid = s.mark(grid, t_sorted, s.S_f, valid)
    index, count = s.compact(valid)
    raw_f, save_f = s.forward_save(pk_f, t_sorted, s.S_f, s.S_f, masked=(index, count), raw=raw_f)
    rgb, depth = s.composite(raw_f, t_sorted, s.S_f, s.S_f)
    stats = getattr(renderer, "masked_stats", None)
    if stats is not None:         # (points the fine network evaluated as a 1-element device tensor, capacity): no host sync here
        stats.append((count.clone(), s.n * s.S_f))
    cap = getattr(renderer, "capture_adjoints", None)
    if cap is not None:
        cap["valid_sorted"] = valid.clone()
    ctx.renderer, ctx.prec, ctx.params = renderer, s.prec, params
    ctx.save_for_backward(rays_o, rays_d, raw_c, save_c, t_sorted, raw_f, save_f, index, count)
    return rgb, depth


def _masked_backward(ctx, g_rgb, g_depth, n_inputs):
    """The backward of such a step; the parameters are the inputs from `n_inputs` on."""
    rays_o, rays_d, raw_c, save_c, t_sorted, raw_f, save_f, index, count = ctx.saved_tensors
    s = _Step(ctx.renderer, rays_o, rays_d, ctx.prec, ctx.stochastic)
    s.begin_backward(ctx, g_rgb, g_depth, n_inputs)
    if s.grads is None:
        return (None,) * (n_inputs + len(s.params))
    # fine pass: image -> raw_fine and depths (all 192 samples; g_raw is exactly zero at the masked ones: sigma = 0)
    g_raw_f, g_t = s.composite_backward(raw_f, t_sorted, s.S_f, s.S_f)
    g_t.add_(s.mlp_backward_masked(s.params[24:], s.grads[24:], t_sorted, s.S_f, (index, count), g_raw_f, save_f))
    # coarse pass, as in the unmasked step
    s.coarse_backward(raw_c, save_c, t_sorted, g_t, s.live_count(s.S_f))
    return (None,) * n_inputs + s.param_grads()


class MaskedRenderFunction(torch.autograd.Function):
    """The step with fast_sampling: the sampler also yields the validity of the 192 merged samples (coarse samples always valid,
    fine ones unless ESS / ERT / the empty-ray test drop them); the fine network runs on the M valid samples, raw_fine is exactly 0
    at the others (network.py:238-253).  The mask is made of comparisons, a constant for autograd: compositing's adjoint runs over
    all 192 samples, the fine MLP's backward over the M compact rows, and g_t of a masked sample has no point term."""

    @staticmethod
    def forward(ctx, renderer, rays_o, rays_d, *params):
        return _masked_forward(ctx, renderer, rays_o, rays_d, None, None, params)

    @staticmethod
    def backward(ctx, g_rgb, g_depth):
        return _masked_backward(ctx, g_rgb, g_depth, 3)


class CulledRenderFunction(torch.autograd.Function):
    """The step with Renderer.train_occupancy: the coarse pass as in the plain step (unculled, shared or jittered depths), then the
    grid's fine bitfield looked up at the 192 merged depths (nerf_occupancy_mark; ANDed into the sampler's mask with fast_sampling)
    and the fine network on the kept samples only, raw_fine = 0 at the others.  The lookup is made of comparisons, a constant for
    autograd, so the backward is the masked step's, with the stochastic strides when draws are given.  A culled sample with a true
    sigma <= 0 has an exactly zero g_raw row in the plain step too: wherever the grid is right the gradients are the plain step's."""

    @staticmethod
    def forward(ctx, renderer, rays_o, rays_d, draws, grid, *params):
        return _masked_forward(ctx, renderer, rays_o, rays_d, draws, grid, params)

    @staticmethod
    def backward(ctx, g_rgb, g_depth):
        return _masked_backward(ctx, g_rgb, g_depth, 5)


class CoarseRenderFunction(torch.autograd.Function):
    """The step with N_importance == 0 (volume_renderer.py:306-345 returning the coarse outputs): the full coarse network on the
    64 table depths, compositing over them, and the adjoints of both.  The depths are constants, so the MLP backward is asked
    for no g_t.  Only the 24 coarse tensors are inputs: the fine sub-model is unused, its .grad stays None as in the reference."""

    @staticmethod
    def forward(ctx, renderer, rays_o, rays_d, *params):
        s = _Step(renderer, rays_o, rays_d)
        raw_c, save_c = s.forward_save(renderer.net.packed(""), s.t_c, 0, s.S_c)
        rgb, depth = s.composite(raw_c, s.t_c, 0, s.S_c)
        ctx.renderer, ctx.prec, ctx.params = renderer, s.prec, params
        ctx.save_for_backward(rays_o, rays_d, raw_c, save_c)
        return rgb, depth

    @staticmethod
    def backward(ctx, g_rgb, g_depth):
        rays_o, rays_d, raw_c, save_c = ctx.saved_tensors
        s = _Step(ctx.renderer, rays_o, rays_d, ctx.prec)
        s.begin_backward(ctx, g_rgb, g_depth, 3)
        if s.grads is None:
            return (None,) * (3 + len(s.params))
        g_raw_c, _ = s.composite_backward(raw_c, s.t_c, 0, s.S_c, depths=False)
        s.mlp_backward(s.params, s.grads, s.t_c, 0, s.S_c, g_raw_c, save_c, depths=False)
        stats = getattr(ctx.renderer, "live_tile_stats", None)
        if stats is not None:
            stats.append((None, 0, s.live_count(s.S_c), s.n * s.S_c // 32))
        return (None, None, None) + s.param_grads()


def check_differentiable(renderer, rays_grad=False):
    """Raise NotImplementedError for the modes without adjoint kernels (modes.DIFFERENTIABLE): fp16 precisions, and gradients with
    respect to the rays (`rays_grad`) with fast_sampling or N_importance == 0 -- those two modes train their parameters only."""
    modes.resolve(modes.facts(renderer, modes.STEP, rays_grad, 1), table=modes.CHECK_DIFFERENTIABLE)


def _all_params(net):
    return tuple(net.model.ordered_params()) + tuple(net.model_fine.ordered_params())


# the path modes.resolve names -> (renderer, rays_o, rays_d, draws, grid) -> (rgb, depth)
_STEPS = {
    "step": lambda r, o, d, draws, grid: RenderFunction.apply(r, o, d, draws, *_all_params(r.net)),
    "step_masked": lambda r, o, d, draws, grid: MaskedRenderFunction.apply(r, o, d, *_all_params(r.net)),
    "step_coarse": lambda r, o, d, draws, grid: CoarseRenderFunction.apply(r, o, d, *r.net.model.ordered_params()),
    "step_culled": lambda r, o, d, draws, grid: CulledRenderFunction.apply(r, o, d, draws, grid, *_all_params(r.net)),
}


def render_with_grad(renderer, rays_o, rays_d, jitter=None, u=None, occupancy=None):
    """rays [n,3] (contiguous fp32, on the GPU) -> (rgb [n,3], depth [n]) attached to the autograd graph of
    the 48 network parameters (coarse sub-model first, then fine, state_dict order) and of the rays, each where it
    requires grad.  `jitter` [n,64] / `u` [n,128]: the reference's training-mode draws (Renderer._draws); None keeps the
    shared deterministic table.  `occupancy`: an OccupancyGrid whose fine bitfield culls the fine pass (Renderer.render has
    checked it); parameter gradients only, N_importance = 128."""
    draws = (jitter, u) if (jitter is not None or u is not None) else None
    facts = modes.facts(renderer, modes.STEP, rays_o.requires_grad or rays_d.requires_grad, rays_o.shape[0],
                        draws=draws is not None, train_occupancy=occupancy is not None)
    return _STEPS[modes.resolve(facts)](renderer, rays_o, rays_d, draws, occupancy)


class FusedAdam(torch.optim.Optimizer):
    """clip_grad_value_ + Adam in one HIP launch over all parameter tensors of a group (nerf_adam_step).  Same update
    as torch.optim.Adam(lr, eps, weight_decay) of src/train/optimizer.py:21-24 preceded by trainer.py:59's
    clip_grad_value_(40).  It IS a torch.optim.Optimizer (param_groups, state, state_dict in torch.optim.Adam's layout),
    so the reference's schedulers (ExponentialLR / MultiStepLR of src/utils/optimizer/lr_scheduler.py, built by
    make_lr_scheduler) and its save_model / load_model (net_utils.py:288-343) drive it unchanged, and a checkpoint
    moves freely between this optimizer and torch.optim.Adam.

    The arithmetic is fp32 in the operation order of torch's device kernels, every operation rounded on its own, with the constants
    formed in double on the host, as torch forms them from these Python floats (1 - beta1, 1 - beta2, sqrt(1 - beta2^step),
    -(lr / (1 - beta1^step)), each rounded to fp32 once; include/nerf_mi355x.h has the formulas).  Both forms of torch's lerp are
    followed, so beta1 <= 0.5 is served.  A NaN gradient stays NaN through the clip, as clamp_ leaves it, and makes its parameter
    NaN; +-inf is clipped.  Parameters whose grad is None are left alone with their state; a zero-element parameter is stepped
    over.  tests/adam_reference.py restates the step; tests/test_gpu_adam.py holds the kernel to it bit for bit."""

    def __init__(self, params, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_value=40.0):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, clip_value=clip_value,
                        amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__([p for p in params if not isinstance(p, torch.Tensor) or p.requires_grad], defaults)
        for g in self.param_groups:
            if len(g["params"]) > 48:
                raise ValueError("FusedAdam handles at most 48 tensors per parameter group (one launch per group)")

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
            st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
        return st

    # conveniences over param_groups[0] / state (tests, bench)
    @property
    def params(self):
        return [p for g in self.param_groups for p in g["params"]]

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, value):
        for g in self.param_groups:
            g["lr"] = value

    @property
    def clip_value(self):
        return self.param_groups[0]["clip_value"]

    @property
    def exp_avg(self):
        return [self._state_of(p)["exp_avg"] for p in self.params]

    @property
    def exp_avg_sq(self):
        return [self._state_of(p)["exp_avg_sq"] for p in self.params]

    @property
    def step_count(self):
        return max([int(float(self._state_of(p)["step"])) for p in self.params] or [0])

    @step_count.setter
    def step_count(self, value):
        for p in self.params:
            self._state_of(p)["step"] = torch.tensor(float(value))

    @staticmethod
    def exponential_lr(lr0, epoch, gamma=0.1, decay_epochs=500):
        return lr0 * gamma ** (epoch / decay_epochs)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        bump = getattr(torch.autograd.graph, "increment_version", None)
        for g in self.param_groups:
            if g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("FusedAdam does not implement amsgrad / maximize")
            live = [p for p in g["params"] if p.grad is not None]
            if not live:
                continue
            states = [self._state_of(p) for p in live]
            steps = {int(float(st["step"])) for st in states}
            if len(steps) != 1:
                raise ValueError("FusedAdam: tensors of one group are at different steps {}".format(sorted(steps)))
            step = steps.pop() + 1
            dev = live[0].device
            for st in states:                     # state loaded from a CPU checkpoint follows its parameter
                for k in ("exp_avg", "exp_avg_sq"):
                    if st[k].device != dev:
                        st[k] = st[k].to(dev)
            grads = [p.grad.contiguous() for p in live]
            _lib.call("nerf_adam_step", len(live), live, grads, [st["exp_avg"] for st in states], [st["exp_avg_sq"] for st in states],
                      [p.numel() for p in live], float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                      float(g["weight_decay"]), float(g.get("clip_value", 40.0)), step)
            for p, st in zip(live, states):
                st["step"] = torch.tensor(float(step))
                # the packed weight streams are keyed on (data_ptr, _version): tell autograd the HIP kernel wrote in
                # place, so Network.packed() repacks (cache invalidation only, no kernel launched)
                if bump is not None:
                    bump(p)
                else:
                    p.add_(0)
        return loss


def train_step(renderer, optimizer, rays_o, rays_d, colors, clip_value=40.0, group=None, time=None):
    """One step of the reference's intended loop (trainer.py:53-60 with trainers/nerf.py:27-33): render,
    MSE on the fine RGB, backward, [data-parallel: one gradient all-reduce], clip_grad_value_(40),
    optimizer.step().  Returns the loss tensor.  time (None, or the frame number per ray [n]): passed on as
    batch["time"], which a HashRenderer over a dynamic field needs."""
    from .dist import allreduce_gradients
    optimizer.zero_grad(set_to_none=True)
    batch = {"rays_o": rays_o[None], "rays_d": rays_d[None]}
    if time is not None:
        batch["time"] = time[None]
    rgb, _ = renderer.render(batch)
    loss = torch.nn.functional.mse_loss(rgb, colors)
    loss.backward()
    allreduce_gradients(renderer.net.parameters(), group)
    if not isinstance(optimizer, FusedAdam):          # FusedAdam clips inside its kernel
        torch.nn.utils.clip_grad_value_(renderer.net.parameters(), clip_value)
    optimizer.step()
    return loss.detach()
