"""conv3x3(nearest_upsample_2x(x)) as four 2 x 2 phase convolutions (csrc/ops_gemm.hip: nk_conv2d_up2_*), the three identities in float64 on
the CPU against F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1) and its autograd:

  * forward: phase (a, b) of y is the 2 x 2 / stride 1 convolution of x with top / left padding (1 - a, 1 - b) and the summed weights wp;
  * input gradient: one 4 x 4 / stride 2 / padding 1 convolution of dy with the table wd;
  * weight gradient: the four phase convolutions' weight gradients folded back onto the nine taps, the bias gradient their sum.

The index formulas here are the ones the kernels implement (up2_phase_weights_kernel, Up2FoldWgrad, PixelShuffle2x); the GPU test
(tests/test_up2_phases_gpu.py) checks the kernels against the fused-gather path and this reference."""
import pytest
import torch
import torch.nn.functional as F

# (N, H, W, Cin, Cout): H or W = 1, odd sizes, one pixel
SHAPES = [(1, 1, 1, 3, 2), (2, 1, 5, 2, 3), (1, 4, 1, 3, 3), (2, 5, 7, 3, 4), (1, 9, 4, 2, 2), (1, 6, 10, 4, 3)]


def taps_on(a, u):
    """the taps kh of the 3-tap kernel that output row 2i + a applies to low-resolution row i + a - 1 + u"""
    return [kh for kh in range(3) if (a + kh - 1) // 2 == a - 1 + u]


def phase_weights(w):
    """w [Cout, Cin, 3, 3] -> wp [2, 2, Cout, Cin, 2, 2] (a, b, co, ci, u, v)"""
    Cout, Cin = w.shape[:2]
    wp = w.new_zeros(2, 2, Cout, Cin, 2, 2)
    for a in range(2):
        for b in range(2):
            for u in range(2):
                for v in range(2):
                    for kh in taps_on(a, u):
                        for kw in taps_on(b, v):
                            wp[a, b, :, :, u, v] += w[:, :, kh, kw]
    return wp


def dgrad_weights(wp):
    """wd [Cin, Cout, 4, 4] (ci, co, r, s) = wp[(r+1)&1][(s+1)&1][co][ci][1-(r>>1)][1-(s>>1)]"""
    Cout, Cin = wp.shape[2:4]
    wd = wp.new_zeros(Cin, Cout, 4, 4)
    for r in range(4):
        for s in range(4):
            wd[:, :, r, s] = wp[(r + 1) & 1, (s + 1) & 1, :, :, 1 - (r >> 1), 1 - (s >> 1)].t()
    return wd


def fold(dwp):
    """dwp [2, 2, Cout, Cin, 2, 2] -> dw [Cout, Cin, 3, 3]: tap (kh, kw) of phase (a, b) lies on (u, v) = (kh > a, kw > b)"""
    Cout, Cin = dwp.shape[2:4]
    dw = dwp.new_zeros(Cout, Cin, 3, 3)
    for kh in range(3):
        for kw in range(3):
            for a in range(2):
                for b in range(2):
                    dw[:, :, kh, kw] += dwp[a, b, :, :, int(kh > a), int(kw > b)]
    return dw


def phase_conv(x, wpab, a, b):
    """2 x 2 / stride 1 convolution with padding (top, left) = (1 - a, 1 - b) and as many output pixels as input pixels"""
    return F.conv2d(F.pad(x, (1 - b, b, 1 - a, a)), wpab)


def reference(x, w, bias, dy):
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    bias = bias.clone().requires_grad_(True)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, bias, padding=1)
    y.backward(dy)
    return y.detach(), x.grad, w.grad, bias.grad


def case(shape, seed=0):
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    return r(N, Cin, H, W), r(Cout, Cin, 3, 3), r(Cout), r(N, Cout, 2 * H, 2 * W)


def test_tap_sets_are_the_issues_table():
    assert [taps_on(0, 0), taps_on(0, 1), taps_on(1, 0), taps_on(1, 1)] == [[0], [1, 2], [0, 1], [2]]
    # the kernels' closed forms: taps (u ? 1 + a : 0) .. + (u ^ a), and u = kh > a
    for a in range(2):
        for u in range(2):
            lo = 1 + a if u else 0
            assert taps_on(a, u) == list(range(lo, lo + 1 + (u ^ a)))
            assert all(int(kh > a) == u for kh in taps_on(a, u))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_is_four_phase_convolutions(shape):
    x, w, bias, dy = case(shape)
    y = reference(x, w, bias, dy)[0]
    wp = phase_weights(w)
    got = torch.empty_like(y)
    for a in range(2):
        for b in range(2):
            got[:, :, a::2, b::2] = phase_conv(x, wp[a, b], a, b) + bias[None, :, None, None]
    assert torch.allclose(got, y, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_input_gradient_is_one_4x4_stride2_convolution_of_dy(shape):
    x, w, bias, dy = case(shape, 1)
    dx = reference(x, w, bias, dy)[1]
    got = F.conv2d(dy, dgrad_weights(phase_weights(w)), stride=2, padding=1)
    assert got.shape == dx.shape
    assert torch.allclose(got, dx, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_gradient_is_the_fold_of_the_phase_gradients(shape):
    x, w, bias, dy = case(shape, 2)
    _, _, dw, db = reference(x, w, bias, dy)
    N, H, W, Cin, Cout = shape
    dwp = torch.zeros(2, 2, Cout, Cin, 2, 2, dtype=torch.float64)
    dbp = torch.zeros(2, 2, Cout, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            wz = torch.zeros(Cout, Cin, 2, 2, dtype=torch.float64, requires_grad=True)
            phase_conv(x, wz, a, b).backward(dy[:, :, a::2, b::2])
            dwp[a, b] = wz.grad
            dbp[a, b] = dy[:, :, a::2, b::2].sum((0, 2, 3))
    assert torch.allclose(fold(dwp), dw, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dbp.sum((0, 1)), db, rtol=1e-12, atol=1e-12)


def test_fold_is_the_adjoint_of_the_phase_weights():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(3, 2, 3, 3, dtype=torch.float64, generator=g)
    q = torch.randn(2, 2, 3, 2, 2, 2, dtype=torch.float64, generator=g)
    assert torch.allclose((phase_weights(w) * q).sum(), (w * fold(q)).sum(), rtol=1e-12, atol=1e-12)


def test_the_default_takes_the_phase_path_by_size(monkeypatch):
    """NK_UP2_PHASES: unset / 1 = by size (the UNet's two Upsample layers at batch 1 and up; not a toy model's), 0 = never, 2 = always"""
    from neurosis_amd import ops

    unet = [(n * 32 * 32, 1280, 1280) for n in (1, 4)] + [(n * 64 * 64, 640, 640) for n in (1, 4)]
    tiny = [(1, 8, 8), (2 * 8 * 8, 128, 128), (2 * 16 * 16, 64, 64)]
    monkeypatch.delenv("NK_UP2_PHASES", raising=False)
    assert all(ops.up2_phases_take(*s) for s in unet) and not any(ops.up2_phases_take(*s) for s in tiny)
    monkeypatch.setenv("NK_UP2_PHASES", "1")
    assert all(ops.up2_phases_take(*s) for s in unet) and not any(ops.up2_phases_take(*s) for s in tiny)
    monkeypatch.setenv("NK_UP2_PHASES", "0")
    assert not any(ops.up2_phases_take(*s) for s in unet + tiny)
    monkeypatch.setenv("NK_UP2_PHASES", "2")
    assert all(ops.up2_phases_take(*s) for s in unet + tiny)
