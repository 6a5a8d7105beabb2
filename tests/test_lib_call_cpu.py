"""CPU checks of _lib.call, the one path from the package into the C ABI: what it refuses, it refuses before the library is
touched.  Needs the built library, no GPU.  The evidence that no C call was made is nerf_last_error(): every refused C call
overwrites it, a refusal in Python leaves it as it was."""
import pytest
import torch


@pytest.fixture()
def marked_library():
    """The library with a known last error, left by a C call that refuses its sizes without touching a pointer."""
    import nerf_replication_amd._lib as L
    lib = L.load()
    assert lib.nerf_occupancy_age(None, 1, -1, 0.0, 1, None, None, None) == -1
    mark = lib.nerf_last_error()
    assert b"n_points" in mark
    return L, lib, mark


def _refused(L, lib, mark, exc, name, *args):
    with pytest.raises(exc) as info:
        L.call(name, *args)
    assert name in str(info.value)
    assert lib.nerf_last_error() == mark                          # no C call was made
    return str(info.value)


def test_call_refuses_before_the_library(marked_library):
    L, lib, mark = marked_library
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    # a CPU tensor, with the wording ptr() has always used
    msg = _refused(L, lib, mark, L.NerfLibraryError, "nerf_composite", f(3, 64, 4), f(64), 0, 3, 64, 1, f(3, 3), f(3), None)
    assert "needs tensors on a GPU (cuda) device; got a CPU tensor" in msg and "argument 0" in msg
    # 2 arguments to a 9-argument entry
    assert len(L.SIGNATURES["nerf_composite"][1]) == 9 + 1        # + the stream, which call supplies
    msg = _refused(L, lib, mark, TypeError, "nerf_composite", f(3, 64, 4), f(64))
    assert "9 arguments (2 given)" in msg
    # a host array of the wrong length: 11 doubles for c2w[12]
    msg = _refused(L, lib, mark, L.NerfLibraryError, "nerf_generate_rays", [0.0] * 11, 4, 4, 1.0, 0, 16, None, f(16, 3), f(16, 3))
    assert "argument 0" in msg and "12" in msg and "11" in msg
    # a host array of device pointers of the wrong length: 23 tensors for params[24]
    msg = _refused(L, lib, mark, L.NerfLibraryError, "nerf_pack_model", [f(4)] * 23, torch.zeros(8, dtype=torch.uint8), 0)
    assert "argument 0" in msg and "24" in msg and "23" in msg


def test_call_refusals_do_not_load_the_library(monkeypatch):
    """The same order seen from the other side: with load() replaced, a refused call never reaches it (call looks `load` up in the
    module at call time)."""
    import nerf_replication_amd._lib as L
    monkeypatch.setattr(L, "load", lambda: pytest.fail("argument errors must not reach the library"))
    with pytest.raises(L.NerfLibraryError):
        L.call("nerf_positional_encoding", torch.zeros(5, 3), 5, 10, torch.zeros(5, 63))
    with pytest.raises(TypeError):
        L.call("nerf_positional_encoding")
    with pytest.raises(L.NerfLibraryError):
        L.call("nerf_occupancy_build", L.strided(torch.zeros(3, 3, 3, 4)[..., 3]), 4, 3, 3, 3, 0.0, 0, torch.zeros(2, dtype=torch.int32))


def test_size_queries_return_their_value(marked_library):
    """Return kinds other than a status come back unchanged: -1 is the caller's to handle, nothing is raised."""
    L, lib, _ = marked_library
    assert L.call("nerf_train_save_floats", -1) == -1
    assert L.call("nerf_packed_model_bytes", 7) == -1
    assert L.call("nerf_packed_model_bytes", L.PREC_F32X) == lib.nerf_packed_model_bytes(L.PREC_F32X) > 0
    assert L.call("nerf_abi_version") == 3
    assert isinstance(L.call("nerf_last_error"), bytes)


def test_protos_are_the_ctypes_view_of_the_table():
    import ctypes
    import nerf_replication_amd._lib as L
    assert tuple(L._PROTOS) == L.EXPORTS == tuple(L.SIGNATURES)
    res, args = L._PROTOS["nerf_occupancy_mark"]
    assert res is ctypes.c_int32 and args[3] is ctypes.c_int64 and args[6] is ctypes.c_void_p and args[-1] is ctypes.c_void_p
    assert args[7] is ctypes.POINTER(ctypes.c_int32) and args[8] is ctypes.POINTER(ctypes.c_float)
    assert L._PROTOS["nerf_pack_model"][1][0] is ctypes.POINTER(ctypes.c_void_p)
    assert L._PROTOS["nerf_last_error"] == (ctypes.c_char_p, [])
    assert L._PROTOS["nerf_generate_rays"][1][0] is ctypes.POINTER(ctypes.c_double)
