"""CPU: the size entries of the C ABI.  Every workspace is one layout struct, carved once on the caller's pointer and once on a
null base for its *_workspace_bytes entry; the values here are those of the hand-written size formulas the structs replaced, so
a layout that grows, shrinks or reorders a piece shows up without a GPU."""
import pytest


@pytest.fixture(scope="module")
def lib():
    import nerf_replication_amd._lib as L
    L.build()
    return L.load()


def test_render_workspace_bytes(lib, monkeypatch):
    monkeypatch.delenv("NERF_RENDER_BLOCK_RAYS", raising=False)
    got = [lib.nerf_render_workspace_bytes(n, n_imp, fast) for n in (1, 4096, 640000, 1 << 21) for n_imp in (0, 128) for fast in (0, 1)]
    assert got == [1536, 1536, 5376, 6144, 4210944, 4210944, 19939584, 23855360, 657920256, 657920256, 3115520256, 3727360256,
                   1077936384, 1077936384, 5104468224, 6106906880]
    got = [lib.nerf_render_stochastic_workspace_bytes(n, n_imp) for n in (1, 4096, 1 << 21) for n_imp in (0, 128)]
    assert got == [1792, 5632, 5259520, 20988160, 1346371840, 5372903680]
    got = [lib.nerf_render_occupancy_workspace_bytes(n, n_imp, fast) for n in (1, 4096) for n_imp in (0, 128) for fast in (0, 1)]
    assert got == [2048, 2048, 6656, 6656, 5521664, 5521664, 25166080, 25166080]


def test_training_workspace_bytes(lib):
    assert [lib.nerf_compact_valid_workspace_bytes(n) for n in (0, 1, 256, 257, 786432, -1, 1 << 31)] == [0, 256, 256, 256, 12288, -1, -1]
    assert [lib.nerf_mlp_backward_masked_workspace_bytes(n) for n in (0, 32, 786432, -1)] == [0, 1536, 31457280, -1]
    assert lib.nerf_density_gradient_point_bytes() == 20224


def test_geometry_workspace_bytes(lib):
    dims = ((0, 0, 0), (2, 2, 2), (67, 63, 66), (256, 256, 256), (2048, 2048, 2048))
    assert [lib.nerf_isosurface_workspace_bytes(*d) for d in dims] == [0, 768, 1123584, 67633152, -1]
    sizes = ((0, 0), (1, 0), (1000, 3000), (3000, 1000), (-1, 0))
    assert [lib.nerf_mesh_components_workspace_bytes(v, t) for v, t in sizes] == [0, 1024, 16640, 36352, -1]
