"""The banded resampler (csrc/resample.hip) as antialiased bicubic resize: ops.resize_bicubic_aa forward and backward against float64
`F.interpolate(mode="bicubic", antialias=True)` and its autograd on the CPU.

The bound is derived, not tuned.  With fp32-rounded weights (relative error 2^-24 each) and fp32 fma chains of t_v and t_h links over the
two passes, the first-order error of one output is at most (t_v + t_h + 4) * 2^-24 * |Wv|_inf * |Wh|_inf * max|x| (one rounding per
link, one per weight and per stored intermediate and output; the row-L1 norms bound the magnitudes that are rounded); a factor 2 covers the
higher-order terms.  The norms come from the float64 matrices.  Tables computed in fp32, or weights evaluated in fp32, do not meet it:
torch's own fp32 CPU result misses float64 by 3e-8 .. 2.4e-5 on these shapes."""
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [
    ((2, 3, 13, 37), (7, 19)),          # odd sizes, clipped windows
    ((2, 3, 24, 20), (10, 36)),         # one axis down, the other up
    ((1, 3, 8, 8), (16, 16)),           # upscale
    ((1, 3, 10, 10), (24, 24)),         # upscale
    ((1, 2, 64, 64), (5, 5)),           # long tap loops
    ((1, 2, 5, 5), (64, 64)),           # long tap loops in the transposed tables
    ((1, 1, 2, 2), (5, 5)),             # every window clipped on both sides
    ((1, 3, 16, 16), (16, 16)),         # must return the input unchanged
    ((2, 3, 512, 512), (224, 224)),     # multi-workgroup; the DreamSim backbones' shape
]
IDS = [f"{'x'.join(map(str, s))}-to-{'x'.join(map(str, o))}" for s, o in SHAPES]
EPS = 2.0 ** -24


def _bound(n_in_v, n_out_v, n_in_h, n_out_h, transposed, amax):
    from neurosis_amd.resample import axis_bands, axis_matrix

    Mv, Mh = axis_matrix(n_in_v, n_out_v), axis_matrix(n_in_h, n_out_h)
    bv, bh = axis_bands(n_in_v, n_out_v)[int(transposed)], axis_bands(n_in_h, n_out_h)[int(transposed)]
    if transposed:
        Mv, Mh = Mv.T, Mh.T
    nv, nh = np.abs(Mv).sum(axis=1).max(), np.abs(Mh).sum(axis=1).max()
    return 2.0 * (bv.taps + bh.taps + 4) * EPS * nv * nh * amax


@lru_cache(maxsize=None)
def _case(i):
    """inputs, the float64 references and the two bounds of SHAPES[i]; computed once, shared, never modified"""
    shape, out = SHAPES[i]
    g = torch.Generator().manual_seed(1234 + i)
    x = torch.rand(shape, generator=g) * 2.0 - 1.0
    dy = torch.rand(shape[:2] + out, generator=g) * 2.0 - 1.0
    xd = x.double().requires_grad_(True)
    ref = F.interpolate(xd, size=out, mode="bicubic", antialias=True)
    (ref_dx,) = torch.autograd.grad(ref, xd, dy.double())
    H, W = shape[2:]
    b_fwd = _bound(H, out[0], W, out[1], False, float(x.abs().max()))
    b_bwd = _bound(H, out[0], W, out[1], True, float(dy.abs().max()))
    return x, dy, ref.detach(), ref_dx, b_fwd, b_bwd


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_forward_against_float64_interpolate(i):
    from neurosis_amd import ops

    x, _, ref, _, b_fwd, _ = _case(i)
    xg = x.cuda()
    y, _ = ops.resize_bicubic_aa(xg, SHAPES[i][1])
    if SHAPES[i][0][2:] == SHAPES[i][1]:
        assert y is xg
    assert y.shape == ref.shape and y.dtype == torch.float32
    err = float((y.cpu().double() - ref).abs().max())
    print(f"forward {IDS[i]}: max error {err:.3e}, bound {b_fwd:.3e}")
    assert err <= b_fwd, (err, b_fwd)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_backward_against_float64_autograd(i):
    from neurosis_amd import ops

    x, dy, _, ref_dx, _, b_bwd = _case(i)
    _, bwd = ops.resize_bicubic_aa(x.cuda(), SHAPES[i][1])
    dx = bwd(dy.cuda())
    assert dx.shape == x.shape and dx.dtype == torch.float32
    err = float((dx.cpu().double() - ref_dx).abs().max())
    print(f"backward {IDS[i]}: max error {err:.3e}, bound {b_bwd:.3e}")
    assert err <= b_bwd, (err, b_bwd)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_backward_is_the_adjoint_of_forward(i):
    """<R x, g> = <x, R^T g>, both sides accumulated in float64 from the fp32 results, relative to |R x| |g|"""
    from neurosis_amd import ops

    x, dy, _, _, b_fwd, b_bwd = _case(i)
    y, bwd = ops.resize_bicubic_aa(x.cuda(), SHAPES[i][1])
    dx = bwd(dy.cuda())
    yd, gd = y.cpu().double(), dy.double()
    lhs, rhs = float((yd * gd).sum()), float((x.double() * dx.cpu().double()).sum())
    rel = abs(lhs - rhs) / float(yd.norm() * gd.norm())
    print(f"adjointness {IDS[i]}: {rel:.3e}, bound {b_fwd + b_bwd:.3e}")
    assert rel <= b_fwd + b_bwd, (lhs, rhs, rel)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_bit_identical_from_run_to_run_and_through_the_torch_ops(i):
    import neurosis_amd.torch_ops  # noqa: F401  (registers torch.ops.neurosis_hip.*)
    from neurosis_amd import ops

    x, dy, _, _, _, _ = _case(i)
    (H, W), (OH, OW) = SHAPES[i][0][2:], SHAPES[i][1]
    xg, dyg = x.cuda(), dy.cuda()
    y1, bwd1 = ops.resize_bicubic_aa(xg, (OH, OW))
    y2, bwd2 = ops.resize_bicubic_aa(xg, (OH, OW))
    assert torch.equal(y1, y2)
    d1, d2 = bwd1(dyg), bwd2(dyg)
    assert torch.equal(d1, d2)
    assert torch.equal(torch.ops.neurosis_hip.resize_bicubic_aa(xg, OH, OW), y1)
    assert torch.equal(torch.ops.neurosis_hip.resize_bicubic_aa_bwd(dyg, H, W), d1)
    assert torch.equal(ops.resize_bicubic_aa_bwd(dyg, (H, W)), d1)


def test_the_torch_op_is_differentiable_and_refuses_what_the_kernel_does_not_take():
    import neurosis_amd.torch_ops  # noqa: F401
    from neurosis_amd import ops

    x, dy, _, _, _, _ = _case(0)
    xg = x.cuda().requires_grad_(True)
    y = torch.ops.neurosis_hip.resize_bicubic_aa(xg, *SHAPES[0][1])
    (got,) = torch.autograd.grad(y, xg, dy.cuda())
    assert torch.equal(got, ops.resize_bicubic_aa(x.cuda(), SHAPES[0][1])[1](dy.cuda()))
    with pytest.raises(ValueError):
        ops.resize_bicubic_aa(x.cuda().to(torch.bfloat16), (7, 19))
    with pytest.raises(ValueError):
        ops.resize_bicubic_aa(x.cuda(), (7, 19))[1](dy.cuda()[:, :, :-1])
    # a non-contiguous view is made dense, not misread
    wide = torch.rand(2, 3, 13, 40, device="cuda") * 2 - 1
    assert torch.equal(ops.resize_bicubic_aa(wide[..., :37], (7, 19))[0], ops.resize_bicubic_aa(wide[..., :37].contiguous(), (7, 19))[0])
