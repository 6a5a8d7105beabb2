"""Renderer with the reference's plugin surface (src/models/nerf/renderer/volume_renderer.py:8-24,
:290-432): ``Renderer(net).render(batch) -> (rgb [B*N,3], depth [B*N])``, executed by the HIP
kernels behind include/nerf_mi355x.h.

Loadable through the reference's loader (src/models/nerf/renderer/make_renderer.py:4-8), see
INTEGRATION.md.  Hyper-parameters follow the reference's *effective* behaviour:
N_samples 64, N_importance 128, near/far 2/6, white background.  Sampling is deterministic unless the reference's
training mode is selected (cfg.task == "train": jittered coarse depths if perturb, random inverse-CDF u); its random numbers
are the one ATen op on that path (Renderer._rand, see README "Stochastic sampling").
"""
import os
import sys

import torch


def _sibling(name):
    """Import a sibling module of this package by its absolute name.  The reference loads this file by PATH
    (imp.load_source(cfg.*_module, cfg.*_path), make_network.py:4-8 / make_renderer.py:4-8), under whatever dotted name
    the YAML gives and with the CWD -- not necessarily sys.path -- holding the package directory."""
    import importlib
    try:
        return importlib.import_module("nerf_replication_amd." + name)
    except ModuleNotFoundError as exc:
        if exc.name != "nerf_replication_amd":
            raise
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        return importlib.import_module("nerf_replication_amd." + name)


_lib = _sibling("_lib")
modes = _sibling("modes")


def _reference_cfg():
    mod = sys.modules.get("src.config")
    return getattr(mod, "cfg", None) if mod is not None else None


UNIT_ORDER_SAMPLE_RAYS = 16          # rays of the call that calibration evaluates: indices floor((2 k + 1) n / 32)
UNIT_ORDER_MIN_RAYS = 160000         # 4 x (one-off cost 7.1 ms / gain 0.180 us per ray) = 158 k rays, LAB_NOTEBOOK.md "unit orders"


class Renderer:
    def __init__(self, net):
        cfg = _reference_cfg()
        self.net = net
        # same getattr-on-top-level-cfg reads as volume_renderer.py:14-24 (they normally miss -> defaults)
        self.N_samples = getattr(cfg, "N_samples", 64)
        self.chunk_size = getattr(cfg, "chunk_size", 1024)
        self.white_bkgd = getattr(cfg, "white_bkgd", True)
        self.N_importance = getattr(cfg, "N_importance", 128)
        self.sample_size = 64
        self.rays_size = 160000
        self.task = getattr(cfg, "task", "test")
        self.perturb = bool(getattr(cfg, "perturb", True)) if self.task == "train" else False
        self.fast_sampling = getattr(cfg, "fast_sampling", False)
        self.weights_threshold = getattr(cfg, "weights_threshold", 0.25)
        self.t_near, self.t_far = 2.0, 6.0            # default args of the stratified sampler (:27)
        self.device = None
        self._tables = {}
        self._workspace = None
        # occupancy culling (occupancy.py): an OccupancyGrid, or None = every sample is evaluated.  occupancy_stats: set it
        # to a list to receive (evaluated [2] int64 device tensor, (64 n, 192 n)) per culled render() call, without a host sync
        self.occupancy = None
        self.occupancy_stats = None
        # training with a grid: an OccupancyGrid whose FINE bitfield culls the fine pass of the training step (its coarse
        # bitfield is ignored), refreshed from the network every train_occupancy_every steps once the parameters moved.  Read at render()
        # time; acts on the autograd path only (inference culling is `occupancy`)
        self.train_occupancy = None
        self.train_occupancy_every = 16
        # render_geometry works ray block by ray block: a block's scratch is ~3.9 MB per ray (the saved rows and gradient
        # rows of its 192 points), so 4096 rays -- a training step's batch -- are about 16 GB
        self.geometry_block_rays = 4096
        # unit orders: "auto" = the second fp32 no-grad render() of one weights version with at least
        # unit_order_min_rays rays calibrates an order on 16 of its rays, and from then on the whole-frame launches read the
        # ordered stream (Network.packed_inference) for as long as the weights stay; a first large call alone is no sign that the
        # weights will be rendered again.  "off" (or NERF_UNIT_ORDER=0 in the environment) = the identity stream, always.  The
        # threshold is four times the number of rays whose gain pays for one calibration (measured, LAB_NOTEBOOK "unit orders"):
        # a small call never pays it
        self.unit_order = "auto"
        self.unit_order_min_rays = UNIT_ORDER_MIN_RAYS
        if self.N_samples != _lib.N_SAMPLES or self.N_importance not in (0, _lib.N_IMPORTANCE):
            raise ValueError("HIP renderer is built for N_samples=64 and N_importance in {0,128}")

    # host-built, bit-sensitive tables: torch.linspace on the CPU, then copied
    def _get_tables(self, dev):
        tabs = self._tables.get(dev)
        if tabs is None:
            t_c = torch.linspace(self.t_near, self.t_far, self.N_samples).to(dev)
            u = torch.linspace(0.0, 1.0, steps=_lib.N_IMPORTANCE).to(dev)
            tabs = self._tables[dev] = (t_c, u)
        return tabs

    def _rand(self, shape, device):
        """The reference's random draws (volume_renderer.py:59, :145): torch.rand on the rays' device, so torch.manual_seed
        controls the samples.  Overridable: tests replay recorded draws through it."""
        return torch.rand(*shape, device=device)

    def _draws(self, n, dev):
        """(jitter [n,64] or None, u [n,128] or None) of one render() call, drawn in the reference's order: the coarse jitter
        first (if perturb), then the fine u (if task == "train" and there is a fine pass).  Read from the instance at
        render() time, as the reference does."""
        jitter = self._rand((n, self.N_samples), dev).to(torch.float32).contiguous() if self.perturb else None
        u = None
        if self.task == "train" and self.N_importance > 0:
            u = self._rand((n, self.N_importance), dev).to(torch.float32).contiguous()
        return jitter, u

    def _get_workspace(self, nbytes, dev):
        ws = self._workspace
        if ws is None or ws.device != dev or ws.numel() < nbytes:
            self._workspace = None
            ws = self._workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return ws

    def _scheduled_grid(self):
        """The grid of an accepted training call with self.train_occupancy set, after the refresh schedule: one build serves
        train_occupancy_every steps, and a grid whose network did not move is never rebuilt."""
        grid = self.train_occupancy
        if grid.stale(self.net, "fine") and grid.uses >= self.train_occupancy_every:
            grid.refresh(self.net, models=("fine",))
        grid.uses += 1
        return grid

    def render(self, batch):
        rays_o, rays_d = batch["rays_o"], batch["rays_d"]
        self.device = dev = rays_o.device
        if dev.type != "cuda":
            raise _lib.NerfLibraryError("Renderer.render needs rays on a GPU: the render path is HIP-only")
        B, N, _ = rays_o.shape
        n = B * N
        # rays that require grad stay in the graph (pose refinement): reshape / cast / contiguous map the gradient back to [B,N,3]
        rays_grad = torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad)
        if not rays_grad:
            rays_o, rays_d = rays_o.detach(), rays_d.detach()
        o = rays_o.reshape(n, 3).to(torch.float32).contiguous()
        d = rays_d.reshape(n, 3).to(torch.float32).contiguous()
        facts = modes.facts(self, modes.RENDER, rays_grad, n)
        path = modes.resolve(facts, self, dev)                              # every refusal comes before any launch
        grid = self._scheduled_grid() if facts.with_grad and facts.train_occupancy else None
        draws = self._draws(n, dev) if facts.stochastic else ()
        return self._RENDER[path](self, facts, o, d, draws, grid)

    def _empty(self, facts, o, d, draws, grid):
        if facts.with_grad:
            return torch.empty((0, 3), device=o.device), torch.empty((0,), device=o.device)
        return self._frame_arguments(facts, o, d)[-2:]

    def _step(self, facts, o, d, draws, grid):
        """A training call (trainers/nerf.py:27 under trainer.py:53-60), or rays that require grad: forward with activation save,
        backward through the adjoint HIP kernels (training.py)."""
        kw = {} if grid is None else {"occupancy": grid}
        return _sibling("training").render_with_grad(self, o, d, *draws, **kw)

    # ---- unit orders
    def _unit_order_on(self):
        if self.unit_order not in ("auto", "off"):
            raise ValueError(f"Renderer.unit_order must be 'auto' or 'off', got {self.unit_order!r}")
        return (self.unit_order == "auto" and os.environ.get("NERF_UNIT_ORDER") != "0"
                and _lib.PRECISIONS[modes.precision_of(self.net)] == _lib.PREC_F32)

    def _models(self):
        return ("", "fine") if self.N_importance > 0 else ("",)

    def _inference_streams(self, o=None, d=None):
        """(coarse, fine or None): the streams of the no-grad render launches.  With rays (the whole-frame paths of render()) a
        call of at least unit_order_min_rays rays, when an earlier such call read the same weights, first calibrates whatever
        model has no order for them -- never while the stream is capturing: a capture uses what exists."""
        if not self._unit_order_on():
            return self.net.packed(""), self.net.packed("fine") if self.N_importance > 0 else None
        if (o is not None and o.shape[0] >= self.unit_order_min_rays and not torch.cuda.is_current_stream_capturing()
                and any(self.net.unit_order(m) is None for m in self._models())
                and all([self.net.rendered_before(m) for m in self._models()])):
            self._calibrate(o, d)
        return self.net.packed_inference(""), self.net.packed_inference("fine") if self.N_importance > 0 else None

    def calibrate_unit_order(self, batch):
        """Calibrate the unit orders of the current weights on 16 rays of `batch` now, whatever its size (render() does it by
        itself from unit_order_min_rays rays on).  fp32 only, never during a graph capture; returns the {model: order} set."""
        if modes.precision_of(self.net) not in ("f32", "fp32"):
            raise NotImplementedError("unit orders exist for precision 'f32' only")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("calibrate_unit_order synchronises: not during a graph capture")
        rays_o, rays_d = batch["rays_o"], batch["rays_d"]
        o = rays_o.detach().reshape(-1, 3).to(torch.float32).contiguous()
        d = rays_d.detach().reshape(-1, 3).to(torch.float32).contiguous()
        if o.shape[0] == 0:
            raise ValueError("calibrate_unit_order needs at least one ray")
        return self._calibrate(o, d)

    def _calibrate(self, o, d):
        """16 rays of the call through the render's own stages on the IDENTITY streams, with activation save: coarse forward ->
        nerf_sample_fine -> fine forward; per model the co-dead counts of its 32-sample tiles (nerf_unit_order_stats), the
        matching on the host (nerf_unit_order_match) and the order handed to the network.  One synchronisation (the counts come
        to the host); the ~45 MB of saved rows are freed on return."""
        import ctypes
        n, dev = o.shape[0], o.device
        k = UNIT_ORDER_SAMPLE_RAYS
        # (row copies, not an index kernel: calibration launches nothing of ATen's, whose first use in a process costs far more
        # than everything here)
        os_, ds_ = torch.empty((k, 3), dtype=torch.float32, device=dev), torch.empty((k, 3), dtype=torch.float32, device=dev)
        for i in range(k):
            r = (2 * i + 1) * n // (2 * k)
            os_[i].copy_(o[r])
            ds_[i].copy_(d[r])
        t_c, u = self._get_tables(dev)
        prec = _lib.PREC_F32
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        S_c, S = _lib.N_SAMPLES, _lib.N_SAMPLES + _lib.N_IMPORTANCE
        counts = {}
        raw_c, save = new(k, S_c, 4), new(int(_lib.call("nerf_train_save_floats", k * S_c)))
        _lib.call("nerf_mlp_forward_rays_save", os_, ds_, t_c, 0, k, S_c, self.net.packed(""), raw_c, save, prec)
        counts[""] = torch.empty((8, 256, 256), dtype=torch.int32, device=dev)
        _lib.call("nerf_unit_order_stats", save, k * S_c, counts[""])
        if self.N_importance > 0:
            t_sorted, raw_f = new(k, S), new(k, S, 4)
            _lib.call("nerf_sample_fine", raw_c, t_c, u, k, t_sorted, None, None, 0.0, 0.0)
            save = None
            save = new(int(_lib.call("nerf_train_save_floats", k * S)))
            _lib.call("nerf_mlp_forward_rays_save", os_, ds_, t_sorted, S, k, S, self.net.packed("fine"), raw_f, save, prec)
            counts["fine"] = torch.empty((8, 256, 256), dtype=torch.int32, device=dev)
            _lib.call("nerf_unit_order_stats", save, k * S, counts["fine"])
        orders = {}
        for model, c in counts.items():
            host = c.cpu().numpy()
            order = torch.empty((8, 256), dtype=torch.int32)
            for l in range(8):
                out = (ctypes.c_int32 * 256)()
                _lib.check(_lib.call("nerf_unit_order_match", (ctypes.c_int32 * 65536).from_buffer(host[l]), out),
                           "nerf_unit_order_match")
                order[l] = torch.tensor(list(out), dtype=torch.int32)
            self.net.set_unit_order(model, order)
            orders[model] = self.net.unit_order(model)
        return orders

    def _frame_arguments(self, facts, o, d):
        """What the three whole-frame entries have in common: (rays, models, tables), (modes), fast, and the outputs."""
        n, dev = o.shape[0], o.device
        t_c, u = self._get_tables(dev)
        pk_c, pk_f = self._inference_streams(o, d)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        depth = torch.empty((n,), dtype=torch.float32, device=dev)
        fast = int(bool(self.fast_sampling) and self.N_importance > 0)       # (0 when stochastic: refused)
        modes_ = (int(self.N_importance), int(bool(self.white_bkgd)), _lib.PRECISIONS[facts.precision], fast, float(self.weights_threshold))
        return (o, d, n, pk_c, pk_f, t_c, u), modes_, fast, rgb, depth

    def _frame(self, facts, o, d, draws, grid):
        head, modes_, fast, rgb, depth = self._frame_arguments(facts, o, d)
        ws = self._get_workspace(int(_lib.call("nerf_render_workspace_bytes", head[2], self.N_importance, fast)), o.device)
        _lib.call("nerf_render_forward", *head, *modes_, ws, ws.numel(), rgb, depth)
        return rgb, depth

    def _frame_stochastic(self, facts, o, d, draws, grid):
        head, modes_, _, rgb, depth = self._frame_arguments(facts, o, d)
        ws = self._get_workspace(int(_lib.call("nerf_render_stochastic_workspace_bytes", head[2], self.N_importance)), o.device)
        _lib.call("nerf_render_forward_stochastic", *head, *draws, *modes_, ws, ws.numel(), rgb, depth)
        return rgb, depth

    def _frame_occupancy(self, facts, o, d, draws, grid):
        head, modes_, fast, rgb, depth = self._frame_arguments(facts, o, d)
        n, occ = head[2], self.occupancy
        occ_c, occ_f = occ.bits[""], occ.bits["fine"] if self.N_importance > 0 else None
        ws = self._get_workspace(int(_lib.call("nerf_render_occupancy_workspace_bytes", n, self.N_importance, fast)), o.device)
        evaluated = torch.empty(2, dtype=torch.int64, device=o.device) if self.occupancy_stats is not None else None
        _lib.call("nerf_render_forward_occupancy", *head, *modes_, occ_c, occ_f, *occ.lookup_args(), evaluated, ws, ws.numel(),
                  rgb, depth)
        if evaluated is not None:
            self.occupancy_stats.append((evaluated.clone(), (_lib.N_SAMPLES * n, (_lib.N_SAMPLES + _lib.N_IMPORTANCE) * n)))
        return rgb, depth

    # the path modes.resolve names -> what runs it
    _RENDER = {"empty": _empty, "frame": _frame, "frame_stochastic": _frame_stochastic, "frame_occupancy": _frame_occupancy,
               "step": _step, "step_masked": _step, "step_coarse": _step, "step_culled": _step}

    def render_geometry(self, batch):
        """rgb [n,3] and depth [n] as render(batch) returns them (bit-equal), plus the two other geometry outputs of the composited
        network (fine; coarse when N_importance == 0): acc [n] = sum_i w_i, the accumulated opacity, and normal [n,3] = sum_i w_i n_i
        with n_i = -grad sigma / |grad sigma| at sample i where sigma_i > 0, else 0 (include/nerf_mi355x.h, "geometry outputs").  The
        normal is not renormalised: |normal| <= acc.  white_bkgd does not enter acc or normal.

        Inference only: no autograd path (detached tensors under any grad mode; rays that require grad are refused).  The rays go
        through in blocks of self.geometry_block_rays; the result does not depend on the blocking.  Per block: the staged calls
        nerf_render_forward is made of, then nerf_density_gradient(positive_only) at the composited depths and
        nerf_composite_normals.  Deterministic sampling in precision 'f32' / 'f32x'; see DESIGN section 6 for what is refused."""
        rays_o, rays_d = batch["rays_o"], batch["rays_d"]
        self.device = dev = rays_o.device
        if dev.type != "cuda":
            raise _lib.NerfLibraryError("Renderer.render_geometry needs rays on a GPU: the render path is HIP-only")
        B, N, _ = rays_o.shape
        n = B * N
        facts = modes.facts(self, modes.GEOMETRY, rays_o.requires_grad or rays_d.requires_grad, n)
        path = modes.resolve(facts, self, dev)                              # every refusal comes before any launch
        block = self.geometry_block_rays
        o = rays_o.detach().reshape(n, 3).to(torch.float32).contiguous()
        d = rays_d.detach().reshape(n, 3).to(torch.float32).contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = {"rgb": new(n, 3), "depth": new(n), "acc": new(n), "normal": new(n, 3)}
        if path == "empty":
            return out
        prec = _lib.PRECISIONS[facts.precision]
        t_c, u = self._get_tables(dev)
        fine = self.N_importance > 0
        model = "fine" if fine else ""
        # the forward launches read the streams render() reads (rgb and depth stay bit-equal to it, with or without a unit
        # order; an order is used when one exists, never calibrated here); the gradient chain saves rows in parameter order and
        # stays on the identity stream and its transpose
        pk_c, pk_fwd = self._inference_streams()
        pk_fwd = pk_fwd if fine else pk_c
        pk = self.net.packed(model)
        pk_b = self.net.packed_bwd(model)
        S_c, S = _lib.N_SAMPLES, _lib.N_SAMPLES + (_lib.N_IMPORTANCE if fine else 0)
        nb_max = min(block, n)
        raw_c = new(nb_max, S_c, 4)
        t_sorted, raw_f = (new(nb_max, S), new(nb_max, S, 4)) if fine else (None, None)
        grad = new(nb_max, S, 3)
        ws = torch.empty(int(_lib.call("nerf_density_gradient_point_bytes")) * ((nb_max * S + 31) // 32 * 32), dtype=torch.uint8, device=dev)
        white = int(bool(self.white_bkgd))
        for r0 in range(0, n, block):
            nb = min(block, n - r0)
            ob, db = o[r0:r0 + nb], d[r0:r0 + nb]
            if fine:
                _lib.call("nerf_mlp_forward_rays_density", ob, db, t_c, 0, nb, S_c, pk_c, raw_c, prec)
                _lib.call("nerf_sample_fine", raw_c, t_c, u, nb, t_sorted, None, None, 0.0, 0.0)
                _lib.call("nerf_mlp_forward_rays_for_compositing", ob, db, t_sorted, S, nb, S, pk_fwd, raw_f, prec)
                raw, tv, stride = raw_f, t_sorted, S
            else:
                _lib.call("nerf_mlp_forward_rays", ob, db, t_c, 0, nb, S_c, pk_c, raw_c, prec)
                raw, tv, stride = raw_c, t_c, 0
            _lib.call("nerf_composite", raw, tv, stride, nb, S, white, out["rgb"][r0:r0 + nb], out["depth"][r0:r0 + nb], None)
            _lib.call("nerf_density_gradient", ob, db, tv, stride, nb, S, pk, pk_b, 1, None, grad, prec, ws, ws.numel())
            _lib.call("nerf_composite_normals", raw, tv, stride, nb, S, grad, out["normal"][r0:r0 + nb], out["acc"][r0:r0 + nb])
        return out
