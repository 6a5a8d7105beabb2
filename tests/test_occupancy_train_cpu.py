"""CPU checks of training with an occupancy grid: the defaults and refusals of Renderer.train_occupancy
(modes.resolve, before any library call), the refresh schedule with the refresh and the step stubbed, the size checks of nerf_occupancy_age, and the
NumPy restatement tests/occupancy_train_reference.py against its definition.  The kernel and the step are compared on the GPU in
tests/test_gpu_occupancy_train.py."""
import numpy as np
import pytest
import torch

import occupancy_train_reference as A

BOX = [-2.0, -2.0, -2.0, 2.0, 2.0, 2.0]
DIMS = (5, 6, 7)


def _grid(pkg, net=None, fine=True, coarse=False, device="cpu"):
    """An OccupancyGrid without a GPU: zeroed words of the right count; with `net`, the keys from_network would record."""
    from nerf_replication_amd.occupancy import OccupancyGrid, _params_key
    n_cells = (DIMS[0] - 1) * (DIMS[1] - 1) * (DIMS[2] - 1)
    words = lambda: torch.zeros(2 * ((n_cells + 63) // 64), dtype=torch.int32)
    bits = {"": words() if coarse else None, "fine": words() if fine else None}
    keys = None if net is None else {m: _params_key(net, m) for m in bits if bits[m] is not None}
    grid = OccupancyGrid(np.asarray(BOX, dtype=np.float64).reshape(2, 3), DIMS, 0.0, 1, bits, keys)
    grid.device = torch.device(device)
    return grid


def test_defaults():
    import nerf_replication_amd as pkg
    r = pkg.Renderer(pkg.Network())
    assert r.train_occupancy is None and r.train_occupancy_every == 16
    assert r.occupancy is None
    grid = _grid(pkg)
    assert grid.hold == 1 and grid.uses == 0


def test_refusals_come_before_any_library_call(monkeypatch):
    """The checks of a training call with a grid, in their order, each one launch-free: the library is not even loaded."""
    import nerf_replication_amd as pkg
    from nerf_replication_amd import modes
    monkeypatch.setattr(pkg._lib, "load", lambda: pytest.fail("refusals must not reach the library"))
    net = pkg.Network()
    cpu = torch.device("cpu")
    r = pkg.Renderer(net)
    grid = _grid(pkg, net)

    def train_call(dev, rays_grad):
        """What render() does with a training call before the step: resolve, then the grid's schedule."""
        path = modes.resolve(modes.facts(r, modes.RENDER, rays_grad, 8), r, dev)
        return path, r._scheduled_grid()

    def refused(exc, rays_grad=False, dev=cpu):
        with pytest.raises(exc):
            train_call(dev, rays_grad)
        assert grid.uses == 0                                      # a refused call does not count as a step

    for bad in ("grid", 3, object()):
        r.train_occupancy = bad
        refused(TypeError)
    r.train_occupancy = grid
    for bad_every in (0, -1, 2.0, "4", None, True):
        r.train_occupancy_every = bad_every
        refused(ValueError)
    r.train_occupancy_every = 16
    r.train_occupancy = _grid(pkg, net, fine=False, coarse=True)     # no fine bitfield
    refused(ValueError)
    r.train_occupancy = grid
    refused(ValueError, dev=torch.device("cuda", 0))               # the grid is elsewhere
    refused(NotImplementedError, rays_grad=True)
    r.N_importance = 0
    refused(NotImplementedError)
    r.N_importance = 128
    # the existing checks come first: an fp16 network is refused as it is without a grid, whatever the grid is
    for precision in ("f16", "f16m32"):
        net.precision = precision
        r.train_occupancy = "grid"
        refused(NotImplementedError)
    net.precision = "f32"
    r.train_occupancy = grid
    assert train_call(cpu, False) == ("step_culled", grid) and grid.uses == 1    # nothing to refuse, not stale: no refresh, one use

    # hold is validated by refresh, before the library and before the network is looked at
    for bad_hold in (0, 256, -1, 1.5, "2", None, True):
        grid.hold = bad_hold
        with pytest.raises(ValueError):
            grid.refresh(net)
    grid.hold = 255
    with pytest.raises(TypeError):
        grid.refresh(object())
    for bad_models in ((), ("medium",), ("fine", "fine"), 3):
        with pytest.raises(ValueError):
            grid.refresh(net, models=bad_models)
    with pytest.raises(ValueError):
        grid.refresh(net, models=("",))                             # this grid has no coarse bitfield


def test_age_entry_refuses_sizes_without_a_gpu():
    """The size and range checks come first and touch neither a pointer nor the device."""
    import nerf_replication_amd._lib as L
    lib = L.load()
    assert "nerf_occupancy_age" in L.EXPORTS
    assert lib.nerf_occupancy_age(None, 1, -1, 0.0, 1, None, None, None) == -1
    assert lib.nerf_occupancy_age(None, 1, 1 << 31, 0.0, 1, None, None, None) == -1
    assert b"n_points" in lib.nerf_last_error()
    assert lib.nerf_occupancy_age(None, 1, 8, 0.0, 0, None, None, None) == -1
    assert lib.nerf_occupancy_age(None, 1, 8, 0.0, 256, None, None, None) == -1
    assert b"hold" in lib.nerf_last_error()
    assert lib.nerf_occupancy_age(None, 0, 8, 0.0, 1, None, None, None) == -1              # stride < 1
    assert lib.nerf_occupancy_age(None, 1, 0, 0.0, 1, None, None, None) == 0               # no points: a no-op
    assert lib.nerf_occupancy_age(None, 1, 0, 0.0, 255, None, None, None) == 0
    assert lib.nerf_occupancy_age(None, 1, 0, 0.0, 0, None, None, None) == -1              # the range check even then
    assert lib.nerf_occupancy_age(None, 1, 8, 0.0, 1, None, None, None) == -1              # null pointers


class _FakeRays:
    """What Renderer.render asks of its rays before it hands them to the step, without a GPU."""
    device, requires_grad, shape = torch.device("cuda", 0), False, (1, 8, 3)

    def detach(self):
        return self

    def reshape(self, *a):
        return self

    def to(self, *a):
        return self

    def contiguous(self):
        return self


def _scheduled_run(monkeypatch, every, bump, net_keys=True, calls=10):
    """`calls` training calls of render() with the step and the refresh stubbed -> (the calls (1-based) a refresh came before,
    the grids the step was handed, the grid)."""
    import nerf_replication_amd as pkg
    from nerf_replication_amd import occupancy, training
    net = pkg.Network()
    assert net.training
    grid = _grid(pkg, net if net_keys else None, device="cuda:0")
    r = pkg.Renderer(net)
    r.train_occupancy, r.train_occupancy_every = grid, every
    refreshed, handed, call = [], [], [0]

    def refresh(self, network, models=None):
        assert self is grid and network is net and models == ("fine",)
        refreshed.append(call[0])
        self.keys["fine"] = occupancy._params_key(network, "fine")
        self.uses = 0

    def step(renderer, o, d, jitter=None, u=None, occupancy=None):
        handed.append(occupancy)
        return torch.zeros(8, 3), torch.zeros(8)

    monkeypatch.setattr(occupancy.OccupancyGrid, "refresh", refresh)
    monkeypatch.setattr(training, "render_with_grad", step)
    for i in range(calls):
        call[0] = i + 1
        r.render({"rays_o": _FakeRays(), "rays_d": _FakeRays()})
        if bump:
            with torch.no_grad():
                net.model_fine.alpha_linear.bias.add_(0.0)           # an in-place update, as an optimizer step is
    return refreshed, handed, grid


def test_schedule(monkeypatch):
    refreshed, handed, grid = _scheduled_run(monkeypatch, every=4, bump=True)
    assert refreshed == [5, 9]                                      # one build serves 4 steps
    assert len(handed) == 10 and all(g is grid for g in handed)
    assert grid.uses == 2
    refreshed, _, grid = _scheduled_run(monkeypatch, every=4, bump=False)
    assert refreshed == [] and grid.uses == 10                      # the parameters did not move
    refreshed, _, _ = _scheduled_run(monkeypatch, every=4, bump=True, net_keys=False)
    assert refreshed == []                                          # a grid from fields is never stale
    refreshed, _, _ = _scheduled_run(monkeypatch, every=1, bump=True)
    assert refreshed == list(range(2, 11))                          # before every step whose parameters changed
    refreshed, _, _ = _scheduled_run(monkeypatch, every=16, bump=True, calls=18)
    assert refreshed == [17]


def test_schedule_only_on_the_autograd_path(monkeypatch):
    """Under no_grad the attribute is not even looked at: render() goes on to the inference path."""
    import nerf_replication_amd as pkg
    from nerf_replication_amd import training
    r = pkg.Renderer(pkg.Network())
    r.train_occupancy = "not a grid"
    monkeypatch.setattr(training, "render_with_grad", lambda *a, **k: pytest.fail("not a training call"))

    class Inference(Exception):
        pass

    def tables(dev):
        raise Inference

    monkeypatch.setattr(r, "_get_tables", tables)                   # the first thing the inference path does
    with torch.no_grad(), pytest.raises(Inference):
        r.render({"rays_o": _FakeRays(), "rays_d": _FakeRays()})
    r.net.eval()
    with pytest.raises(Inference):
        r.render({"rays_o": _FakeRays(), "rays_d": _FakeRays()})


# ---- the restatement against its definition
def test_restatement_age_saturates_and_resets():
    age = A.new_age(3)
    assert age.dtype == np.uint8 and (age == 255).all()
    f = np.array([-1.0, -1.0, 1.0], np.float32)
    age, on = A.age_step(f, 0.0, 255, age)
    assert age.tolist() == [255, 255, 0] and on.tolist() == [-1.0, -1.0, 1.0]          # 255 stays 255: no wrap to 0
    age = np.array([253, 254, 0], np.uint8)
    for expect in ([254, 255, 1], [255, 255, 2], [255, 255, 3]):
        age, on = A.age_step(np.full(3, -1.0, np.float32), 0.0, 255, age)
        assert age.tolist() == expect
    assert on.tolist() == [-1.0, -1.0, 1.0]                         # 255 < hold never holds, 3 < 255 does
    age, on = A.age_step(np.array([1.0, -1.0, -1.0], np.float32), 0.0, 4, age)
    assert age.tolist() == [0, 255, 4] and on.tolist() == [1.0, -1.0, -1.0]            # age == hold: dropped


def test_restatement_nan_is_a_hit_and_level_is_strict():
    f = np.array([np.nan, 0.5, 0.5000001, -np.inf, np.inf], np.float32)
    age, on = A.age_step(f, 0.5, 1, A.new_age(5))
    assert age.tolist() == [0, 255, 0, 255, 0] and on.tolist() == [1.0, -1.0, 1.0, -1.0, 1.0]
    assert on.dtype == np.float32 and age.dtype == np.uint8


def test_restatement_hold_1_is_the_hit_and_hold_2_the_union():
    rng = np.random.default_rng(11)
    fields = [rng.standard_normal((4, 5, 6)).astype(np.float32) for _ in range(4)]
    fields[1][1, 2, 3] = np.nan
    hits = [((f > 0) | np.isnan(f)).reshape(-1) for f in fields]
    for hold in (1, 2, 3):
        age = A.new_age(fields[0].size)
        for i, f in enumerate(fields):
            before = age.copy()
            age, on = A.age_step(f, 0.0, hold, age)
            assert np.array_equal(before, before.copy()) and set(np.unique(on)) <= {-1.0, 1.0}
            union = np.zeros_like(hits[0])
            for h in hits[max(0, i - hold + 1):i + 1]:               # the last `hold` refreshes, the first ones look back on nothing
                union |= h
            assert np.array_equal(on > 0, union), (hold, i)
