"""Host side of the antialiased bicubic resize: the float64 tables of neurosis_amd/resample.py against the matrix torch itself applies
(recovered from `F.interpolate(mode="bicubic", antialias=True)` on float64 impulses), the banded storage and its transpose, and the op
surface (schemas, Meta shapes, CPU tensors refused).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from neurosis_amd import resample as R

PAIRS = [(13, 7), (37, 19), (24, 10), (20, 36), (8, 16), (10, 24), (64, 5), (5, 64), (2, 5), (512, 224), (16, 16)]


def torch_matrix(n_in: int, n_out: int) -> np.ndarray:
    """[n_out, n_in] float64: column j is torch's response to the impulse at j (the resize acts on the height axis; width 2 is untouched)"""
    eye = torch.eye(n_in, dtype=torch.float64).reshape(n_in, 1, n_in, 1).expand(n_in, 1, n_in, 2).contiguous()
    out = F.interpolate(eye, size=(n_out, 2), mode="bicubic", antialias=True)
    assert torch.equal(out[..., 0], out[..., 1])
    return out[:, 0, :, 0].T.numpy()


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_axis_matrix_is_torchs(n_in, n_out):
    M = R.axis_matrix(n_in, n_out)
    assert M.dtype == np.float64 and M.shape == (n_out, n_in)
    assert np.abs(M - torch_matrix(n_in, n_out)).max() <= 1e-12
    assert np.abs(M.sum(axis=1) - 1.0).max() <= 1e-14            # every window sums to 1
    if n_in == n_out:
        assert np.array_equal(M, np.eye(n_in))


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_bands_hold_the_matrix_and_its_transpose(n_in, n_out):
    M = R.axis_matrix(n_in, n_out)
    fwd, tr = R.axis_bands(n_in, n_out)
    for band, D in ((fwd, M), (tr, M.T)):
        assert band.start.dtype == np.int32 and band.count.dtype == np.int32 and band.weights.dtype == np.float32
        assert (band.n_out, band.n_in) == D.shape and band.weights.shape == (D.shape[0], band.taps)
        assert (band.start >= 0).all() and (band.count >= 1).all() and (band.start + band.count <= band.n_in).all()
        assert band.taps == int(band.count.max())                 # max_taps is the true maximum, not an upper estimate
        assert np.array_equal(band.dense(), D.astype(np.float32).astype(np.float64))      # nothing outside the windows, fp32 rounding only
        for i in range(band.n_out):
            assert not band.weights[i, band.count[i]:].any()      # rows padded with zeros
    assert np.abs(fwd.weights.astype(np.float64).sum(axis=1) - 1.0).max() <= 4 * fwd.taps * 2.0 ** -24
    assert np.array_equal(tr.dense(), fwd.dense().T)              # the transposed table IS the matrix transpose, bit for bit
    # windows move monotonically: that is what makes the transpose banded
    assert (np.diff(fwd.start) >= 0).all() and (np.diff(tr.start) >= 0).all()


def test_tap_counts_of_the_extreme_ratios():
    assert R.axis_bands(64, 5)[0].taps == 52 and R.axis_bands(5, 64)[1].taps == 52
    assert R.axis_bands(512, 224)[0].taps == 10
    with pytest.raises(ValueError):
        R.axis_matrix(0, 4)


def test_torch_ops_have_schemas_and_meta_kernels():
    import neurosis_amd.torch_ops as T

    assert {"resize_bicubic_aa", "resize_bicubic_aa_bwd"} <= set(T.OPS)
    assert str(torch.ops.neurosis_hip.resize_bicubic_aa.default._schema) == "neurosis_hip::resize_bicubic_aa(Tensor x, SymInt out_h, SymInt out_w) -> Tensor"
    assert str(torch.ops.neurosis_hip.resize_bicubic_aa_bwd.default._schema) == "neurosis_hip::resize_bicubic_aa_bwd(Tensor dy, SymInt in_h, SymInt in_w) -> Tensor"
    x = torch.empty(2, 3, 13, 37, device="meta")
    y = torch.ops.neurosis_hip.resize_bicubic_aa(x, 7, 19)
    assert y.shape == (2, 3, 7, 19) and y.dtype == torch.float32 and y.device.type == "meta"
    dx = torch.ops.neurosis_hip.resize_bicubic_aa_bwd(y, 13, 37)
    assert dx.shape == x.shape and dx.device.type == "meta"
    with pytest.raises(NotImplementedError):                      # no CPU dispatch key: torch's own error
        torch.ops.neurosis_hip.resize_bicubic_aa(torch.zeros(1, 1, 4, 4), 2, 2)


def test_cpu_tensors_are_refused():
    from neurosis_amd import lib, ops

    with pytest.raises(NotImplementedError, match="no CPU path"):
        ops.resize_bicubic_aa(torch.zeros(1, 3, 8, 8), (4, 4))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ops.resize_bicubic_aa(torch.zeros(1, 3, 8, 8), (8, 8))    # also where the sizes agree
    with pytest.raises(NotImplementedError, match="no CPU path"):
        ops.resize_bicubic_aa_bwd(torch.zeros(1, 3, 4, 4), (8, 8))
    assert "nk_resample_planes" in lib.SIGNATURES and "nk_resample_ws_floats" in lib.SIZE_QUERIES
    # the workspace is the smaller of the two possible intermediates
    assert lib.query("nk_resample_ws_floats", 6, 512, 512, 224, 224) == 6 * 224 * 512
    assert lib.query("nk_resample_ws_floats", 6, 24, 20, 10, 36) == 6 * 10 * 20
    assert lib.query("nk_resample_ws_floats", 2, 5, 5, 64, 64) == 2 * 5 * 64
