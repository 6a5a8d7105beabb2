"""GPU checks of _lib.call: CUDA tensors of the wrong element type or layout are refused before any launch, and what goes
through call is bit-equal to the direct ctypes path (load() + ptr + check, as bench.py calls the C ABI)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import nerf_replication_amd._lib as lib_module
    lib_module.load()
    return lib_module


def _dev():
    return torch.device("cuda", 0)


def test_call_refuses_cuda_tensors_of_the_wrong_kind(L):
    dev = _dev()
    lib = L.load()
    assert lib.nerf_occupancy_age(None, 1, -1, 0.0, 1, None, None, None) == -1
    mark = lib.nerf_last_error()                                  # a refused C call would overwrite it
    f = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    i32 = lambda *shape: f(*shape, dtype=torch.int32)

    def refused(name, *args):
        with pytest.raises(L.NerfLibraryError) as info:
            L.call(name, *args)
        assert name in str(info.value) and lib.nerf_last_error() == mark
        return str(info.value)

    # int64 faces [2,3] where the entry reads int32
    faces = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int64, device=dev)
    ws = f(max(1, L.call("nerf_mesh_components_workspace_bytes", 4, 2)), dtype=torch.uint8)
    labels = (i32(4), i32(2), i32(4), i32(4), i32(4), i32(1))
    assert "argument 0" in refused("nerf_mesh_components", faces, 2, 4, ws, *labels)
    # a float64 raw
    raw, t = torch.randn(3, 64, 4, device=dev), torch.linspace(2.0, 6.0, 64).to(dev)
    rgb, depth = f(3, 3), f(3)
    assert "argument 0" in refused("nerf_composite", raw.double(), t, 0, 3, 64, 1, rgb, depth, None)
    # a transposed (non-contiguous) [3,5] input
    x = torch.rand(5, 3, device=dev)
    pe = f(5, 63)
    assert not x.t().is_contiguous() and x.t().shape == (3, 5)
    assert "argument 0" in refused("nerf_positional_encoding", x.t(), 5, 10, pe)
    # a pointer array holding one fp16 tensor
    params = [f(4), f(4, dtype=torch.float16)]
    others = [[f(4), f(4)] for _ in range(3)]
    assert "argument 1" in refused("nerf_adam_step", 2, params, *others, [4, 4], 1e-3, 0.9, 0.999, 1e-8, 0.0, 40.0, 1)

    # the same tensors' device still serves valid calls
    L.call("nerf_mesh_components", faces.to(torch.int32), 2, 4, ws, *labels)
    L.call("nerf_composite", raw, t, 0, 3, 64, 1, rgb, depth, None)
    L.call("nerf_positional_encoding", x, 5, 10, pe)
    params[1] = f(4)
    L.call("nerf_adam_step", 2, params, *others, [4, 4], 1e-3, 0.9, 0.999, 1e-8, 0.0, 40.0, 1)
    torch.cuda.synchronize(dev)
    assert labels[5].item() == 1 and labels[0].tolist() == [0, 0, 0, 0]           # one component: the two faces share an edge
    assert torch.isfinite(rgb).all() and torch.equal(pe[:, :3], x)


def test_call_is_bit_equal_to_the_direct_path(L):
    dev = _dev()
    lib, st = L.load(), L.stream_of(dev)
    g = torch.Generator().manual_seed(5)
    # positional encoding: 5 points, 10 frequencies
    x = torch.rand(5, 3, generator=g).to(dev)
    a, b = torch.empty(5, 63, device=dev), torch.empty(5, 63, device=dev)
    L.check(lib.nerf_positional_encoding(L.ptr(x), 5, 10, L.ptr(a), st), "nerf_positional_encoding")
    L.call("nerf_positional_encoding", x, 5, 10, b)
    assert torch.equal(a, b)
    # compositing: 3 rays x 64 samples, a shared depth table
    raw, t = torch.randn(3, 64, 4, generator=g).to(dev), torch.linspace(2.0, 6.0, 64).to(dev)
    outs = [[torch.empty(3, 3, device=dev), torch.empty(3, device=dev), torch.empty(3, 64, device=dev)] for _ in range(2)]
    L.check(lib.nerf_composite(L.ptr(raw), L.ptr(t), 0, 3, 64, 1, *[L.ptr(o) for o in outs[0]], st), "nerf_composite")
    L.call("nerf_composite", raw, t, 0, 3, 64, 1, *outs[1])
    assert all(torch.equal(p, q) for p, q in zip(*outs))
    # occupancy build: channel 3 of a [3,3,3,4] raw buffer read in place through strided, against the same grid copied dense
    buf = torch.randn(3, 3, 3, 4, generator=g).to(dev)
    field = buf[..., 3]
    assert not field.is_contiguous() and field.stride(2) == 4
    words = int(L.call("nerf_occupancy_words", 3, 3, 3))
    bits = [torch.full((words,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
    dense = field.contiguous()
    L.check(lib.nerf_occupancy_build(dense.data_ptr(), 1, 3, 3, 3, 0.0, 0, bits[0].data_ptr(), st), "nerf_occupancy_build")
    L.call("nerf_occupancy_build", L.strided(field), 4, 3, 3, 3, 0.0, 0, bits[1])
    L.call("nerf_occupancy_build", dense, 1, 3, 3, 3, 0.0, 0, bits[2])
    assert torch.equal(bits[0], bits[1]) and torch.equal(bits[0], bits[2])
    with pytest.raises(L.NerfLibraryError):                       # without the mark, a strided view is refused
        L.call("nerf_occupancy_build", field, 4, 3, 3, 3, 0.0, 0, bits[1])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="the mixed-device refusal needs two GPUs: this is the one case of this "
                                                          "module that may skip")
def test_call_refuses_tensors_on_two_devices(L):
    d0, d1 = torch.device("cuda", 0), torch.device("cuda", 1)
    x, out = torch.rand(5, 3, device=d0), torch.empty(5, 63, device=d1)
    with pytest.raises(L.NerfLibraryError) as info:
        L.call("nerf_positional_encoding", x, 5, 10, out)
    assert "nerf_positional_encoding" in str(info.value) and "argument 3" in str(info.value)
    z = lambda d: torch.zeros(4, device=d)
    with pytest.raises(L.NerfLibraryError):                       # the elements of a pointer array count too
        L.call("nerf_adam_step", 2, [z(d0), z(d1)], [z(d0), z(d0)], [z(d0), z(d0)], [z(d0), z(d0)], [4, 4],
               1e-3, 0.9, 0.999, 1e-8, 0.0, 40.0, 1)
    # a call on the device that is not current runs there
    out1 = torch.empty(5, 63, device=d1)
    L.call("nerf_positional_encoding", x.to(d1), 5, 10, out1)
    L.call("nerf_positional_encoding", x, 5, 10, out0 := torch.empty(5, 63, device=d0))
    assert torch.equal(out0.cpu(), out1.cpu())
