"""tests/pack_reference.py checked against plain linear algebra, without a GPU: the fold region of the packed fp32 model
(csrc/nerf_layout.h kFold*) is pinned bit for bit against this reference on the GPU (test_gpu_parity.py::
test_pack_matches_layout_reference), so a transposed or mis-permuted reference is caught here first."""
import numpy as np
import pytest

import pack_reference as pr


@pytest.mark.parametrize("prefix", ["model", "model_fine"])
def test_fold_reference_is_the_float64_product(synthetic_sd, prefix):
    """Wvf and bvf, read back out of the reference's packed model in natural order, equal float32(Wv[:, :256] . Wf) and
    float32(Wv[:, :256] . bf + bv) of a float64 matmul to within 1 fp32 ulp.  The two differ only in the order of 256 float64
    additions of exact products: at most about 256 x 2^-53 of the sum of magnitudes before the one rounding to fp32, which can move
    the rounded value by one ulp at a tie and by no more unless the sum cancels to below 2^-21 of its terms.  Measured on this
    checkpoint: 0 ulp for every element of both sub-models."""
    packed = pr.pack_model(synthetic_sd, prefix)
    assert packed.dtype == np.float32 and packed.shape == (pr.OFF_FOLD + pr.FOLD_FLOATS,) == (636224,)
    assert pr.OFF_FOLD * 4 % 256 == 0 and 0 <= pr.OFF_FOLD - pr.UNFOLDED_FLOATS < 64
    Wvf, bvf = pr.unfold(packed)
    assert not np.isnan(Wvf).any() and not np.isnan(bvf).any()                   # every element was placed
    g = lambda n: synthetic_sd[f"{prefix}.{n}"].double()
    Wv, Wf = g("views_linears.0.weight")[:, :256], g("feature_linear.weight")
    want_w = (Wv @ Wf).float().numpy()
    want_b = (Wv @ g("feature_linear.bias") + g("views_linears.0.bias")).float().numpy()
    for got, want in ((Wvf, want_w), (bvf, want_b)):
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
    assert np.abs(want_w).max() > 0 and np.abs(want_b).max() > 0
    # the direction-part blocks are a copy of the stream's own, and everything else in the region is zero
    region = packed[pr.OFF_FOLD:]
    off_views_dir = pr.OFF_HEAD_BIAS - 384 - 256 - 128 - 9 * 256 - 32 * 128
    assert np.array_equal(region[pr.FOLD_OFF_DIR:pr.FOLD_OFF_BIAS], packed[off_views_dir:off_views_dir + 32 * 128])
    assert not region[pr.FOLD_OFF_BIAS + 128:].any() and not packed[pr.UNFOLDED_FLOATS:pr.OFF_FOLD].any()
    assert np.array_equal(packed[pr.OFF_HEAD_BIAS:pr.OFF_HEAD_BIAS + 3], synthetic_sd[f"{prefix}.rgb_linear.bias"].numpy())
