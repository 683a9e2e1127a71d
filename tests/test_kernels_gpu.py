"""Op-level parity of the HIP kernels (through the C-ABI) against plain PyTorch fp32 on the CPU.

Tolerances (stated per SURVEY section 8(c)): kernels read bf16 operands, accumulate in fp32 and write
bf16, so the normalised max error budget per op is 2e-2 (bf16 has 8 significant bits: 2^-8 = 3.9e-3 per
rounding); fp32 outputs (weight gradients, statistics) are held to 1e-2 of their max magnitude because
their bf16 INPUTS are exact in both paths and only the accumulation order differs (observed ~1e-5).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import assert_close, bf16_round

pytestmark = pytest.mark.gpu

TOL_BF16 = 2e-2
TOL_F32 = 1e-2


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


def dev(x, dtype=torch.bfloat16):
    return x.to("cuda", dtype=dtype)


def rnd(*shape, scale=1.0, seed=None):
    g = torch.Generator().manual_seed(seed if seed is not None else (sum(shape) * 7919 + len(shape)))
    return bf16_round(torch.randn(*shape, generator=g) * scale)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 320), (308, 640, 2048), (4, 1280, 320), (1000, 72, 136), (16384, 640, 640),
                                   (32768, 2048, 320), (16300, 4104, 264), (4000, 3600, 328)])  # the last three take the 256x256 kernel (ragged M, N and K)
def test_linear_fwd(ops, M, N, K):
    x, w, b, r = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N), rnd(M, N)
    ref = x @ w.t() + b + r
    got = ops.gemm_nt(dev(x), dev(w), dev(b, torch.float32), dev(r))
    assert_close(got, ref, TOL_BF16, "linear_fwd")


def test_linear_fwd_strided_alpha(ops):
    M, N, K = 200, 96, 64
    xf = rnd(M, 3 * K)
    w = rnd(N, K, scale=0.1)
    x = dev(xf)[:, K:2 * K]
    got = ops.gemm_nt(x, dev(w), alpha=0.25)
    assert_close(got, 0.25 * xf[:, K:2 * K] @ w.t(), TOL_BF16, "linear_fwd strided")


@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (300, 200, 320), (4096, 1280, 640), (8, 1280, 2816),
                                   (4096, 1280, 5120), (4000, 328, 3600)])   # the last two: large grids (ragged M, N, K)
def test_linear_dgrad(ops, M, N, K):
    dy, w, a = rnd(M, N), rnd(N, K, scale=N ** -0.5), rnd(M, K)
    got = ops.gemm_nn(dev(dy), dev(w), dev(a))
    assert_close(got, dy @ w + a, TOL_BF16, "linear_dgrad")


@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (1000, 200, 320), (16384, 640, 640), (308, 1280, 2048), (4, 1280, 320)])
def test_linear_wgrad(ops, M, N, K):
    dy, x = rnd(M, N), rnd(M, K)
    ref = dy.t() @ x
    dw = torch.full((N, K), 7.0, device="cuda")
    ops.gemm_tn_f32(dev(dy), dev(x), dw, False)
    assert_close(dw, ref, TOL_F32, "linear_wgrad store")
    ops.gemm_tn_f32(dev(dy), dev(x), dw, True)
    assert_close(dw, 2 * ref, TOL_F32, "linear_wgrad accumulate")


@pytest.mark.parametrize("M,N,K", [(1000, 200, 320), (4096, 1280, 1280), (4096, 10240, 1280), (308, 1280, 2048), (16384, 640, 640), (4, 1280, 320)])
def test_linear_wgrad_with_fused_bias_gradient(ops, M, N, K):
    """nk_linear_wgrad_bias: the bias gradient (column sums of dy) from the weight-gradient launch itself -- the ring kernel (<= 256 tiles),
    the data-parallel kernel (800 tiles), split-K grids (tiny outputs: fp32 atomics) -- overwrite and accumulate; the weight gradient is
    unchanged bit for bit."""
    dy, x = rnd(M, N), rnd(M, K)
    dyd, xd = dev(dy), dev(x)
    dw_plain = torch.full((N, K), 7.0, device="cuda")
    ops.gemm_tn_f32(dyd, xd, dw_plain, False)
    dw, db = torch.full((N, K), 7.0, device="cuda"), torch.full((N,), -3.0, device="cuda")
    ops.gemm_tn_f32(dyd, xd, dw, False, dbias=db)
    assert_close(dw, dy.t() @ x, TOL_F32, "wgrad")
    if M * 0 + N * K >= 96 * 128 * 128:     # no K split: deterministic, identical to the launch without the bias sum
        assert torch.equal(dw, dw_plain)
    assert_close(db, dy.sum(0), TOL_F32, "fused bias gradient (store)")
    ops.gemm_tn_f32(dyd, xd, dw, True, dbias=db)
    assert_close(db, 2 * dy.sum(0), TOL_F32, "fused bias gradient (accumulate)")
    assert_close(dw, 2 * (dy.t() @ x), TOL_F32, "wgrad accumulate")


# (tokens M, out features N, in features K) -> the 160-row exact-round kernel (csrc/gemm_w160.h) by its shape rule: 256 tiles of 160 x 160,
# 240 of 160 x 128, two whole rounds, and the 64^2-level weights with their token range split over 2 / 4 workgroups (fp32 atomics)
@pytest.mark.parametrize("M,N,K", [(4096, 1280, 5120), (4096, 3840, 1280), (4096, 10240, 1280), (16384, 5120, 640), (16384, 640, 2560)])
def test_linear_wgrad_exact_round_kernel(ops, M, N, K, monkeypatch):
    """Weight gradient + fused bias gradient of the SDXL Linear shapes through nk_gemm_w160_kernel against fp32 on the CPU and against the
    128 x 128 kernels (NK_GEMM_W160=0) -- overwrite, accumulate, and the bias gradient spread over the column tiles."""
    dy, x = rnd(M, N, seed=M + N), rnd(M, K, seed=K + 1)
    dyd, xd = dev(dy), dev(x)
    ref, refb = dy.t() @ x, dy.sum(0)
    dw, db = torch.full((N, K), 7.0, device="cuda"), torch.full((N,), -3.0, device="cuda")
    ops.gemm_tn_f32(dyd, xd, dw, False, dbias=db)
    assert_close(dw, ref, TOL_F32, "w160 wgrad (store)")
    assert_close(db, refb, TOL_F32, "w160 bias gradient (store)")
    ops.gemm_tn_f32(dyd, xd, dw, True, dbias=db)
    assert_close(dw, 2 * ref, TOL_F32, "w160 wgrad (accumulate)")
    assert_close(db, 2 * refb, TOL_F32, "w160 bias gradient (accumulate)")
    monkeypatch.setenv("NK_GEMM_W160", "0")          # read per call by nk_gemm_dispatch
    dw0 = torch.full((N, K), 7.0, device="cuda")
    ops.gemm_tn_f32(dyd, xd, dw0, False)
    monkeypatch.delenv("NK_GEMM_W160")
    dw1 = torch.full((N, K), 7.0, device="cuda")
    ops.gemm_tn_f32(dyd, xd, dw1, False)
    # same bf16 products, fp32 sums in another order: the two kernels agree to fp32 rounding of a 4096-term sum
    assert (dw1 - dw0).abs().max().item() <= 2e-4 * ref.abs().max().item()


@pytest.mark.parametrize("M,N,K,split", [(1000, 200, 320, 1), (300, 168, 136, 1), (2048, 320, 136, 1), (4096, 320, 640, 3), (1030, 488, 200, 2),
                                         (64, 160, 160, 1), (8256, 176, 128, 4)])
def test_linear_wgrad_exact_round_kernel_ragged(ops, M, N, K, split, monkeypatch):
    """NK_GEMM_W160=2 sends EVERY Linear weight gradient to the 160-row kernel: ragged row / column tiles, token counts that are no multiple
    of 64, one-slab reductions, both tile widths, K splits (NK_GEMM_W160_SPLIT: atomics into a zeroed destination) -- with the bias gradient."""
    monkeypatch.setenv("NK_GEMM_W160", "2")
    monkeypatch.setenv("NK_GEMM_W160_SPLIT", str(split))
    dy, x = rnd(M, N, seed=3 * M + N), rnd(M, K, seed=K + 5)
    dyd, xd = dev(dy), dev(x)
    ref, refb = dy.t() @ x, dy.sum(0)
    dw, db = torch.full((N, K), 7.0, device="cuda"), torch.full((N,), -3.0, device="cuda")
    ops.gemm_tn_f32(dyd, xd, dw, False, dbias=db)
    assert_close(dw, ref, TOL_F32, "w160 ragged wgrad (store)")
    assert_close(db, refb, TOL_F32, "w160 ragged bias gradient (store)")
    ops.gemm_tn_f32(dyd, xd, dw, True, dbias=db)
    assert_close(dw, 2 * ref, TOL_F32, "w160 ragged wgrad (accumulate)")
    assert_close(db, 2 * refb, TOL_F32, "w160 ragged bias gradient (accumulate)")
    dw2 = torch.full((N, K), 7.0, device="cuda")
    ops.gemm_tn_f32(dyd, xd, dw2, False)              # without the bias gradient
    assert_close(dw2, ref, TOL_F32, "w160 ragged wgrad, no bias")


@pytest.mark.parametrize("sk_mode", ["1", "2", "3"])
def test_fused_bias_gradient_survives_the_stream_k_switch(ops, sk_mode, monkeypatch):
    """NK_GEMM_SK=1|2|3 routes fp32-output weight gradients to the stream-K kernel, which has no bias row sum: a launch that carries a
    fused bias gradient must stay on a kernel that writes it (round-3 advisor finding: the gradient was silently left unwritten)."""
    M, N, K = 4096, 1280, 640
    dy, x = rnd(M, N), rnd(M, K)
    monkeypatch.setenv("NK_GEMM_SK", sk_mode)        # read per call by nk_gemm_dispatch
    dw, db = torch.full((N, K), 7.0, device="cuda"), torch.full((N,), -3.0, device="cuda")
    ops.gemm_tn_f32(dev(dy), dev(x), dw, False, dbias=db)
    assert_close(dw, dy.t() @ x, TOL_F32, "wgrad under NK_GEMM_SK")
    assert_close(db, dy.sum(0), TOL_F32, "fused bias gradient under NK_GEMM_SK")
    ref = torch.zeros(N, device="cuda")
    ops.colsum(dev(dy), ref, False)
    assert_close(db, ref.cpu(), TOL_F32, "fused bias gradient vs colsum")


@pytest.mark.parametrize("M,N,K,count", [(1024, 256, 384, 3), (64, 128, 128, 8), (4096, 1280, 1280, 3)])
def test_linear_wgrad_batched(ops, M, N, K, count, monkeypatch):
    """`count` same-shape weight gradients in one launch (blockIdx.z) == the launches one by one; also through the queue."""
    assert not ops.state.assume_zeroed and not ops.state.grad_accumulate   # engines keep their flags in their own store.state
    dys, xs = [rnd(M, N) for _ in range(count)], [rnd(M, K) for _ in range(count)]
    q = ops.WgradQueue()
    dws = [torch.full((N, K), 3.0, device="cuda") for _ in range(count)]
    dbs = [torch.full((N,), 5.0, device="cuda") if i != 1 else None for i in range(count)]      # (the second layer has no bias)
    for dy, x, dw, db in zip(dys, xs, dws, dbs):
        q.add(dev(dy), dev(x), dw, db)
    q.add(dev(rnd(M, 2 * N)), dev(rnd(M, K)), torch.zeros(2 * N, K, device="cuda"))  # an odd shape rides along unbatched
    q.flush()
    ops.join_wgrad_stream()
    for dy, x, dw, db in zip(dys, xs, dws, dbs):
        assert_close(dw, dy.t() @ x, TOL_F32, "linear_wgrad_batched")
        if db is not None:
            assert_close(db, dy.sum(0), TOL_F32, "linear_wgrad_batched bias gradient")


def test_colsum(ops):
    dy = rnd(5000, 2560)
    out = torch.zeros(2560, device="cuda")
    ops.colsum(dev(dy), out, False)
    assert_close(out, dy.sum(0), TOL_F32, "colsum")


# ------------------------------------------------------------------------------------------------
def _conv_case(ops, N, H, W, Cin, Cout, k, stride, padding, upsample=False, asym=False, rowvec=False, residual=False):
    x = rnd(N, Cin, H, W)
    w = rnd(Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5)
    b = rnd(Cout)
    xi = x
    if upsample:
        xi = F.interpolate(x, scale_factor=2, mode="nearest")
    if asym:
        xi = F.pad(xi, (0, 1, 0, 1))
    xi = xi.requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    ref = F.conv2d(xi, wr, b, stride=stride, padding=0 if asym else padding)
    rv = rs = None
    if rowvec:
        rv = rnd(N, Cout)
        ref = ref + rv[:, :, None, None]
    if residual:
        rs = rnd(*ref.shape)
        ref = ref + rs
    dy = rnd(*ref.shape)
    ref.backward(dy)

    weight = torch.nn.Parameter(dev(w, torch.float32).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    bias = torch.nn.Parameter(dev(b, torch.float32))
    img = ops.Img(dev(x).permute(0, 2, 3, 1).reshape(-1, Cin).contiguous(), N, H, W)
    rvd = dev(rv) if rv is not None else None
    rsd = dev(rs).permute(0, 2, 3, 1).reshape(-1, Cout).contiguous() if rs is not None else None
    out, bwd = ops.conv2d_fwd(img, weight, bias, stride=stride, padding=padding, upsample=upsample, rowvec=rvd, residual=rsd, asym_pad=asym)
    got = out.t.view(N, out.H, out.W, Cout).permute(0, 3, 1, 2)
    assert got.shape == ref.shape
    assert_close(got, ref, TOL_BF16, "conv fwd")
    dx, drow = bwd(dev(dy).permute(0, 2, 3, 1).reshape(-1, Cout).contiguous())
    dxr = xi.grad
    if asym:
        dxr = dxr[:, :, :-1, :-1]
    if upsample:
        dxr = dxr.view(N, Cin, H, 2, W, 2).sum((3, 5))
    assert_close(dx.t.view(N, H, W, Cin).permute(0, 3, 1, 2), dxr, TOL_BF16, "conv dgrad")
    assert_close(weight.grad, wr.grad, TOL_F32, "conv wgrad")
    assert_close(bias.grad, dy.sum((0, 2, 3)), TOL_F32, "conv bias grad")
    if rowvec:
        assert_close(drow, dy.sum((2, 3)), TOL_BF16, "conv rowvec grad")


def test_conv3x3_s1(ops):
    _conv_case(ops, 2, 16, 16, 64, 128, 3, 1, 1, rowvec=True, residual=True)


def test_conv3x3_ragged(ops):
    _conv_case(ops, 3, 19, 13, 40, 72, 3, 1, 1)


def test_conv3x3_s2(ops):
    _conv_case(ops, 2, 16, 16, 64, 64, 3, 2, 1)


def test_conv3x3_s2_asym(ops):
    _conv_case(ops, 2, 16, 16, 32, 32, 3, 2, 0, asym=True)


def test_conv3x3_upsample(ops):
    _conv_case(ops, 2, 8, 8, 64, 64, 3, 1, 1, upsample=True)


def test_conv3x3_real_channels(ops):
    _conv_case(ops, 1, 32, 32, 320, 320, 3, 1, 1)


def test_conv3x3_big_grid(ops):
    # 131072 output pixels x 128 channels = 512 tiles of 256x128: the ring kernel with the gather loader
    _conv_case(ops, 2, 256, 256, 64, 128, 3, 1, 1, rowvec=True, residual=True)


def test_conv3x3_wide_output(ops):
    # 8192 output pixels x 1920 channels = 256 tiles of 256x256 (the last column tile half empty): the 256x256 kernel with the gather loader
    _conv_case(ops, 2, 64, 64, 64, 1920, 3, 1, 1, rowvec=True, residual=True)


def test_conv4x4_patchgan_shapes(ops):
    # the PatchGAN discriminator's convolutions: 4x4 taps, stride 2 and stride 1, padding 1 (even kernel: asymmetric reach)
    _conv_case(ops, 2, 32, 32, 8, 16, 4, 2, 1)
    _conv_case(ops, 2, 16, 16, 64, 128, 4, 2, 1)
    _conv_case(ops, 2, 8, 8, 32, 64, 4, 1, 1)
    _conv_case(ops, 2, 7, 7, 64, 8, 4, 1, 1)


def test_conv_alexnet_shapes(ops):
    # the LPIPS AlexNet trunk: 11x11 / stride 4 / padding 2 on the (padded) image, and 5x5 / padding 2
    _conv_case(ops, 2, 35, 31, 8, 64, 11, 4, 2)
    _conv_case(ops, 2, 9, 7, 64, 192, 5, 1, 2)


def test_conv3x3_pad_channels(ops):
    # the 4-channel latent convs run with channels padded to 8 (zeros)
    _conv_case(ops, 2, 16, 16, 8, 320, 3, 1, 1)
    _conv_case(ops, 2, 16, 16, 320, 8, 3, 1, 1)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,C,silu,eps", [(2, 16, 16, 320, True, 1e-5), (2, 8, 8, 2560, True, 1e-5), (3, 9, 7, 640, False, 1e-6), (1, 32, 32, 128, True, 1e-6)])
def test_groupnorm(ops, N, H, W, C, silu, eps):
    x = (rnd(N, C, H, W) * 2 + 0.5)
    x = bf16_round(x).requires_grad_(True)
    gamma, beta = rnd(C) * 0.5 + 1, rnd(C) * 0.1
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = F.group_norm(x, 32, gr, br, eps)
    if silu:
        ref = F.silu(ref)
    dy, extra = rnd(N, C, H, W), rnd(N, C, H, W)
    ref.backward(dy)
    w, b = torch.nn.Parameter(dev(gamma, torch.float32)), torch.nn.Parameter(dev(beta, torch.float32))
    tok = lambda t: dev(t.detach()).permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    out, bwd = ops.groupnorm_fwd(ops.Img(tok(x), N, H, W), w, b, 32, eps, silu)
    assert_close(out.t.view(N, H, W, C).permute(0, 3, 1, 2), ref, TOL_BF16, "gn fwd")
    dx = bwd(tok(dy), tok(extra))
    assert_close(dx.view(N, H, W, C).permute(0, 3, 1, 2), x.grad + extra, TOL_BF16, "gn dx")
    assert_close(w.grad, gr.grad, TOL_F32, "gn dgamma")
    assert_close(b.grad, br.grad, TOL_F32, "gn dbeta")


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("M,C", [(1000, 640), (512, 1280), (77, 320), (4100, 1280), (9000, 640), (8, 2048)])
def test_layernorm(ops, M, C, fused, monkeypatch):
    """fused = "1": the one-pass backward (nk_layernorm_bwd_rows + nk_colpart_reduce_batch; a wave walks several rows: 4100 rows = 257 blocks
    with ragged last rows, 9000 rows = the 512-block cap, 8 rows = waves without a row); "0": the three-kernel form"""
    monkeypatch.setenv("NK_LN_FUSED", fused)
    x = bf16_round(rnd(M, C) * 1.5 + 0.3).requires_grad_(True)
    gamma, beta = rnd(C) * 0.5 + 1, rnd(C) * 0.1
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = F.layer_norm(x, (C,), gr, br, 1e-5)
    dy, extra = rnd(M, C), rnd(M, C)
    ref.backward(dy)
    w, b = torch.nn.Parameter(dev(gamma, torch.float32)), torch.nn.Parameter(dev(beta, torch.float32))
    out, bwd = ops.layernorm_fwd(dev(x.detach()), w, b, 1e-5)
    assert_close(out, ref, TOL_BF16, "ln fwd")
    dx = bwd(dev(dy), dev(extra))
    assert_close(dx, x.grad + extra, TOL_BF16, "ln dx")
    ops.join_wgrad_stream()
    assert_close(w.grad, gr.grad, TOL_F32, "ln dgamma")
    assert_close(b.grad, br.grad, TOL_F32, "ln dbeta")


def test_layernorm_partial_rows_reduce_in_one_launch_and_reproducibly(ops):
    """Three LayerNorm backwards hand their partial rows to one WgradQueue (what BasicTransformerBlock.bwd does): one
    nk_colpart_reduce_batch launch writes all six parameter gradients; run twice, the results are bit-identical (fixed fold order), and the
    accumulate flag adds instead of overwriting."""
    M, C = 2048, 640
    outs = []
    for rep in range(2):
        params, refs = [], []
        with ops.batched_wgrads(None) as q:
            for i in range(3):
                x = bf16_round(rnd(M, C, seed=20 + i) + 0.1 * i).requires_grad_(True)
                g0, b0 = (rnd(C, seed=30 + i) * 0.5 + 1).requires_grad_(True), (rnd(C, seed=40 + i) * 0.1).requires_grad_(True)
                dy = rnd(M, C, seed=50 + i)
                F.layer_norm(x, (C,), g0, b0, 1e-5).backward(dy)
                w, b = torch.nn.Parameter(dev(g0.detach(), torch.float32)), torch.nn.Parameter(dev(b0.detach(), torch.float32))
                _, bwd = ops.layernorm_fwd(dev(x.detach()), w, b, 1e-5)
                bwd(dev(dy))
                params.append((w, b))
                refs.append((g0.grad, b0.grad))
            assert q is None or len(q.colparts) == 3
        ops.join_wgrad_stream()
        for (w, b), (gr, br) in zip(params, refs):
            assert_close(w.grad, gr, TOL_F32, "ln dgamma (batched reduce)")
            assert_close(b.grad, br, TOL_F32, "ln dbeta (batched reduce)")
        outs.append([t.grad.clone() for pair in params for t in pair])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,N,I", [(300, 320, 1280), (4096, 1280, 5120), (1000, 136, 264)])
def test_feedforward_out_dgrad_with_fused_geglu_backward(ops, M, N, I):
    """nk_linear_dgrad_geglu: the input gradient of FeedForward.net[2] with the GEGLU backward in the GEMM's epilogue, against autograd
    of (a * gelu(g)) @ W^T on the CPU (ragged M / N / I, the real 1280-wide shape) and against the two separate launches."""
    u = rnd(M, 2 * I).requires_grad_(True)
    w = rnd(N, I, scale=I ** -0.5)
    dy = rnd(M, N)
    a, g = u.chunk(2, dim=-1)
    ((a * F.gelu(g)) @ w.t()).backward(dy)
    ud, wd, dyd = dev(u.detach()), dev(w), dev(dy)
    x = ops.geglu_fwd(ud)[0]
    weight = torch.nn.Parameter(wd.float())
    y, bwd = ops.linear_fwd(x, weight, None)
    fused = bwd(dyd, geglu_u=ud)
    ops.join_wgrad_stream()
    assert fused.shape == (M, 2 * I)
    assert_close(fused, u.grad, TOL_BF16, "fused geglu bwd")
    separate = ops.geglu_fwd(ud)[1](ops.gemm_nn(dyd, ops.w2d(weight)))
    assert_close(fused, separate.float().cpu(), TOL_BF16, "fused vs separate")


@pytest.mark.parametrize("M,N,I", [(300, 320, 1280), (4096, 1280, 5120), (1000, 136, 264)])
def test_feedforward_saved_derivative_form(ops, M, N, I, monkeypatch):
    """Round 6: FeedForward keeps s = [gelu(g) | a gelu'(g)] instead of u = [a | g].  (1) the fused projection's s and h (nk_linear_fwd_geglu_s,
    where the 256 x 256 kernel takes the shape) are bit for bit what nk_geglu_fwd_s makes of the plain projection's u (unrotated k order), and
    equal gelu(g), a gelu'(g) from fp32 autograd at bf16 tolerance; (2) the input gradient of net[2] through s (nk_linear_dgrad_geglu_s) matches
    autograd of (a * gelu(g)) @ W^T and the stand-alone pair nk_linear_dgrad + nk_geglu_bwd_s."""
    K = N
    x, wp_, b = rnd(M, K), rnd(2 * I, K, scale=K ** -0.5), rnd(2 * I, scale=0.1, seed=3)
    wp = torch.nn.Parameter(wp_.float().cuda())
    bp = torch.nn.Parameter(b.cuda())
    monkeypatch.setenv("NK_GEMM_KROT", "0")
    s, h, _ = ops.linear_geglu_fwd(dev(x), wp, bp, save_derivative=True)
    u2, _ = ops.linear_fwd(dev(x), wp, bp)
    h2 = torch.empty_like(h)
    s2 = torch.empty_like(u2)
    ops.call("nk_geglu_fwd_s", u2.data_ptr(), h2.data_ptr(), s2.data_ptr(), M, I, ops._stream())
    assert torch.equal(h, h2) and torch.equal(s, s2)
    assert torch.equal(h, ops.geglu_fwd(u2)[0])                    # the same h as the u-keeping form
    monkeypatch.delenv("NK_GEMM_KROT")
    uq = u2.float().cpu().requires_grad_(True)
    a, g = uq.chunk(2, dim=-1)
    gl = F.gelu(g)
    gl.sum().backward()
    dgelu = uq.grad[:, I:]
    assert_close(s[:, :I], gl.detach(), TOL_BF16, "s1 = gelu(g)")
    assert_close(s[:, I:], (a * dgelu).detach(), TOL_BF16, "s2 = a gelu'(g)")
    # backward through net[2]
    w2, dy = rnd(N, I, scale=I ** -0.5), rnd(M, N, seed=11)
    ur = uq.detach().clone().requires_grad_(True)
    ar, gr = ur.chunk(2, dim=-1)
    ((ar * F.gelu(gr)) @ w2.t()).backward(dy)
    weight2 = torch.nn.Parameter(dev(w2).float())
    y, bwd2 = ops.linear_fwd(h, weight2, None)
    du = bwd2(dev(dy), geglu_s=s)
    ops.join_wgrad_stream()
    assert du.shape == (M, 2 * I)
    assert_close(du, ur.grad, TOL_BF16, "du through the saved-derivative form")
    d = ops.gemm_nn(dev(dy), ops.w2d(weight2))
    du2 = torch.empty_like(du)
    ops.call("nk_geglu_bwd_s", d.data_ptr(), s.data_ptr(), du2.data_ptr(), M, I, ops._stream())
    assert_close(du, du2.float().cpu(), TOL_BF16, "fused vs stand-alone, saved-derivative form")


def test_geglu_silu_add_cat(ops):
    M, I = 300, 2560
    u = rnd(M, 2 * I).requires_grad_(True)
    a, g = u.chunk(2, dim=-1)
    ref = a * F.gelu(g)
    dy = rnd(M, I)
    ref.backward(dy)
    y, bwd = ops.geglu_fwd(dev(u.detach()))
    assert_close(y, ref, TOL_BF16, "geglu fwd")
    assert_close(bwd(dev(dy)), u.grad, TOL_BF16, "geglu bwd")

    x = rnd(4, 1280).requires_grad_(True)
    r = F.silu(x)
    d = rnd(4, 1280)
    r.backward(d)
    y, bwd = ops.silu_fwd(dev(x.detach()))
    assert_close(y, r, TOL_BF16, "silu fwd")
    assert_close(bwd(dev(d)), x.grad, TOL_BF16, "silu bwd")

    p, q = rnd(100, 64), rnd(100, 64)
    assert_close(ops.add(dev(p), dev(q)), p + q, TOL_BF16, "add")

    A, Bc = rnd(2 * 5 * 7, 320), rnd(2 * 5 * 7, 640)
    out, bwd = ops.cat_fwd(ops.Img(dev(A), 2, 5, 7), ops.Img(dev(Bc), 2, 5, 7))
    ref = torch.cat([A, Bc], 1)
    assert torch.equal(out.t.float().cpu(), ref)
    da, db = bwd(out.t)
    assert torch.equal(da.float().cpu(), A) and torch.equal(db.float().cpu(), Bc)


# ------------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, B, H, D):
    Lq, Lk = q.shape[0] // B, k.shape[0] // B
    sp = lambda t, L: t.view(B, L, H, D).transpose(1, 2)
    o = F.scaled_dot_product_attention(sp(q, Lq), sp(k, Lk), sp(v, Lk))
    return o.transpose(1, 2).reshape(B * Lq, H * D)


@pytest.mark.parametrize("B,H,Lq,Lk,D", [(2, 4, 256, 256, 64), (2, 5, 200, 77, 64), (1, 2, 1000, 1000, 64), (2, 3, 130, 77, 40), (1, 2, 96, 96, 160), (1, 1, 64, 200, 80)])
def test_attention(ops, B, H, Lq, Lk, D):
    q, k, v = rnd(B * Lq, H * D), rnd(B * Lk, H * D, seed=5), rnd(B * Lk, H * D, seed=6)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = _attn_ref(qr, kr, vr, B, H, D)
    do = rnd(B * Lq, H * D, seed=9)
    ref.backward(do)
    o, bwd = ops.attention_fwd(dev(q), dev(k), dev(v), B, H, D)
    assert_close(o, ref, TOL_BF16, "attn fwd")
    dq, dk, dv = bwd(dev(do))
    assert_close(dq, qr.grad, TOL_BF16, "attn dq")
    assert_close(dk, kr.grad, TOL_BF16, "attn dk")
    assert_close(dv, vr.grad, TOL_BF16, "attn dv")


@pytest.mark.parametrize("B,H,Lq,Lk,D", [(3, 7, 1000, 1000, 64), (2, 5, 260, 77, 64), (4, 20, 1024, 1024, 64), (2, 3, 130, 300, 40), (1, 11, 200, 200, 160)])
def test_attention_workgroup_order_is_only_an_order(ops, B, H, Lq, Lk, D, monkeypatch):
    """The attention launches are 1-D grids mapped XCD-aware (csrc/attention.hip attn_wg: every XCD owns a contiguous range of (batch, head,
    block), so that the blocks of a head share one L2); NK_ATTN_XCD=0 keeps the 3-D grid.  Every workgroup computes what it computed before:
    forward and all three gradients agree BIT FOR BIT between the two orders -- grids that are and are not multiples of eight, ragged last
    blocks, the one-kernel cross-attention backward, the generic head dims."""
    q, k, v, do = rnd(B * Lq, H * D), rnd(B * Lk, H * D, seed=5), rnd(B * Lk, H * D, seed=6), rnd(B * Lq, H * D, seed=9)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("NK_ATTN_XCD", mode)          # read per launch
        o, bwd = ops.attention_fwd(dev(q), dev(k), dev(v), B, H, D)
        res[mode] = (o.clone(),) + tuple(t.clone() for t in bwd(dev(do)))
    for a, b, name in zip(res["1"], res["0"], ("o", "dq", "dk", "dv")):      # (the query splits of the dK / dV kernel meet in a fixed-order reduce)
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
    assert_close(res["1"][0], _attn_ref(q, k, v, B, H, D), TOL_BF16, "attn fwd, XCD-aware order")


@pytest.mark.parametrize("B,H,Lq,Lk", [(1, 2, 64, 16), (2, 3, 96, 96), (1, 4, 520, 77), (2, 2, 33, 3), (4, 20, 1024, 77), (1, 1, 4100, 80)])
def test_attention_backward_in_one_kernel_for_few_keys(ops, B, H, Lq, Lk, monkeypatch):
    """Head dim 64 with at most 96 keys (the UNet's cross-attention: 77 tokens) runs its whole backward in one kernel (csrc/attention.hip,
    attn64_bwd_small_kernel: keys on lanes in waves 0-2, dS^T through LDS, dQ by wave 3, Q' / -lse2 / -delta made per 32-query tile from rows
    fetched two tiles ahead).  One tile, two, many; one query split and several; ragged last tiles; three keys; a key block that ends
    inside a wave -- against fp32, and against the two-kernel path on the same inputs."""
    D = 64
    q, k, v = rnd(B * Lq, H * D), rnd(B * Lk, H * D, seed=5), rnd(B * Lk, H * D, seed=6)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = _attn_ref(qr, kr, vr, B, H, D)
    do = rnd(B * Lq, H * D, seed=9)
    ref.backward(do)
    o, bwd = ops.attention_fwd(dev(q), dev(k), dev(v), B, H, D)
    dq, dk, dv = bwd(dev(do))
    assert_close(dq, qr.grad, TOL_BF16, "one-kernel dq")
    assert_close(dk, kr.grad, TOL_BF16, "one-kernel dk")
    assert_close(dv, vr.grad, TOL_BF16, "one-kernel dv")
    monkeypatch.setenv("NK_ATTN64_SMALL", "0")          # read per call
    dq2, dk2, dv2 = bwd(dev(do))
    for a, b, name in ((dq, dq2, "dq"), (dk, dk2, "dk"), (dv, dv2, "dv")):
        assert_close(a, b.float().cpu(), 1e-2, f"one-kernel vs two-kernel {name}")


def test_attention_fused_qkv_slices_and_spike(ops):
    """q/k/v as column slices of one buffer; one key spiked so the online-softmax rescale path is taken late."""
    B, H, L, D = 1, 2, 320, 64
    qkv = rnd(B * L, 3 * H * D)
    qkv[300, H * D:2 * H * D] *= 12.0  # a dominant key in the last tile
    q, k, v = qkv.split(H * D, dim=1)
    ref = _attn_ref(q, k, v, B, H, D)
    g = dev(qkv)
    o, _ = ops.attention_fwd(g[:, :H * D], g[:, H * D:2 * H * D], g[:, 2 * H * D:], B, H, D)
    assert_close(o, ref, TOL_BF16, "attn fused-slices")


def _rescale_path_inputs(w_jump, w_keys):
    """Scores that force the data-dependent paths of the head-dim-64 forward: a first tile far BELOW what follows for the u-rows (m must
    rise), u-rows (0, 4, ... of every 32-row wave block) whose scores jump by ~4, ~9 and ~17 log2 units at tiles 2, 4 and 7, w-rows
    (2, 10, ...) that jump by `w_jump` natural units on the keys `w_keys`, and rows that never jump -- all inside one wave block, so a
    wave-uniform decision covers rows that need it and rows that do not."""
    B, H, L, D = 1, 2, 512, 64
    g = torch.Generator().manual_seed(77)
    q = torch.randn(B * L, H, D, generator=g) * 0.5
    k = torch.randn(B * L, H, D, generator=g) * 0.5
    v = torch.randn(B * L, H * D, generator=g)
    # the score of (query, key) rises by  q[3] * k[3] / 8  natural units: the QUERIES carry 32 along dim 3 / 17 and the keys a quarter of the
    # jump (gradients through a large key component against a bf16 dS are dominated by cancellation in any bf16 kernel: with the roles
    # swapped -- queries 8, keys up to 12 -- the generic kernels are 0.2 of the largest dq off)
    q[:, :, 3] = 0.0; q[:, :, 17] = 0.0
    k[:, :, 3] = 0.0; k[:, :, 17] = 0.0
    q[0::4, :, 3] = 32.0
    q[2::8, :, 17] = 32.0
    k[:64, :, 3] = -1.5                    # first tile 6 natural units below for the u-rows
    k[130:134, :, 3] = 0.7                 # ~ +4 log2 units over the running reference at tile 2: deferred, p up to ~2^11
    k[260:262, :, 3] = 1.55                # ~ +9 log2 units at tile 4
    k[w_keys, :, 17] = w_jump / 4
    k[470, :, 3] = 3.0                     # a late jump (+12 natural units) for the u-rows in the last whole tile
    return B, H, L, D, bf16_round(q.reshape(B * L, H * D)), bf16_round(k.reshape(B * L, H * D)), bf16_round(v)


def test_attention_d64_deferred_rescale_paths(ops):
    """The head-dim-64 forward leaves its reference point m alone while a tile's row sums stay under 2^13 and otherwise recomputes the tile
    against a new maximum (csrc/attention.hip, attn64_fwd_kernel).  Both paths are data-dependent and rare on random data, so the inputs
    force them (see _rescale_path_inputs).  Part 1: 32 keys ~9 log2 units up (their SUM crosses the threshold although no single p does),
    forward and backward against fp32 -- the backward consumes the forward's log-sum-exp, so a wrong m / l pairing shows in every gradient.
    Part 2: three keys 28 natural units (40 log2 units) up -- exp2 overflows to +inf in the optimistic pass and the tile must be recomputed."""
    for w_jump, w_keys, tol_dq, tol_dk in ((6.2, slice(384, 416), 8e-2, 8e-2), (28.0, slice(400, 403), 3e-2, TOL_BF16)):
        # (gradient tolerances of the first input: a bf16 dS against |q| = 32 -- with another dO the generic kernels measure 4.9e-2 / 2.6e-2
        # on it, the head-dim-64 ones 4.9e-2 / 3.3e-2 (tools/debug_attn.py); with this dO the latter 5.4e-2 on dk.  The cosine floor of
        # assert_close still holds them to 0.93; measured 0.9998)
        B, H, L, D, q, k, v = _rescale_path_inputs(w_jump, w_keys)
        qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
        ref = _attn_ref(qr, kr, vr, B, H, D)
        do = rnd(B * L, H * D, seed=9)
        ref.backward(do)
        o, bwd = ops.attention_fwd(dev(q), dev(k), dev(v), B, H, D)
        assert_close(o, ref, TOL_BF16, f"attn64 rescale paths fwd ({w_jump})")
        dq, dk, dv = bwd(dev(do))
        assert_close(dq, qr.grad, tol_dq, f"attn64 rescale paths dq ({w_jump})")
        assert_close(dk, kr.grad, tol_dk, f"attn64 rescale paths dk ({w_jump})")
        assert_close(dv, vr.grad, TOL_BF16, f"attn64 rescale paths dv ({w_jump})")


def test_attention_unfused_d512(ops):
    B, L, D = 2, 256, 512
    q, k, v = rnd(B * L, D), rnd(B * L, D, seed=1), rnd(B * L, D, seed=2)
    ref = _attn_ref(q, k, v, B, 1, D)
    got = ops.attention_unfused(dev(q), dev(k), dev(v), B)
    assert_close(got, ref, TOL_BF16, "attn unfused d512")


# ------------------------------------------------------------------------------------------------
def test_layout_and_timestep(ops):
    x = rnd(2, 4, 16, 12)
    t = ops.nchw_to_tokens(dev(x, torch.float32), 8)
    ref = torch.zeros(2, 16, 12, 8)
    ref[..., :4] = x.permute(0, 2, 3, 1)
    assert torch.equal(t.float().cpu().view(2, 16, 12, 8), ref)
    back = ops.tokens_to_nchw(t, 2, 4, 16, 12)
    assert torch.equal(back.cpu(), x)
    big = rnd(2, 70, 9, 5)
    tb = ops.nchw_to_tokens(dev(big), 72)
    assert torch.equal(tb.float().cpu().view(2, 9, 5, 72)[..., :70], big.permute(0, 2, 3, 1))

    ts = torch.tensor([0.0, 1.0, 500.0, 999.0])
    got = ops.timestep_embedding(ts.cuda(), 320)
    half = 160
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)
    args = ts[:, None] * freqs[None]
    ref = torch.cat([torch.cos(args), torch.sin(args)], -1)
    assert float((got.float().cpu() - ref).abs().max()) < 1e-2


def test_stream_k_under_contention(ops, monkeypatch):
    """The persistent stream-K kernel splits tiles across workgroups and joins them through flags.  Run it while another
    stream keeps the CUs busy with ordinary tile-engine kernels (so its 512 workgroups are NOT all resident at once):
    results stay exact w.r.t. the uncontended run and no fix-up wait ever expires."""
    from neurosis_amd import lib

    monkeypatch.setenv("NK_GEMM_SK", "1")
    M, N, K = 4096, 1280, 5120          # 320 tiles x 80 k-steps: every tile is shared by two workgroups
    x, w = dev(rnd(M, K)), dev(rnd(N, K, scale=K ** -0.5))
    want = ops.gemm_nt(x, w).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a, b = dev(rnd(8192, 2048)), dev(rnd(4096, 2048, scale=0.02))
    monkeypatch.setenv("NK_GEMM_SK", "0")
    with torch.cuda.stream(side):
        for _ in range(60):
            ops.gemm_nt(a, b)           # data-parallel kernels, 2 workgroups per CU, on the other stream
    monkeypatch.setenv("NK_GEMM_SK", "1")
    outs = [ops.gemm_nt(x, w) for _ in range(20)]
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, want)     # deterministic fix-up order: bitwise equal
    assert lib.query("nk_gemm_sk_status") == 0


def test_256x256_kernels_agree_bit_for_bit():
    """The two-group phased kernel (Linear forward) against the 128x128 kernels (same accumulation order =>
    identical bits; the Linear dgrad shapes ride along as a stability check), each in its own process over seeded inputs at ragged and full SDXL shapes, repeated under load from a second
    stream: tools/race_screen_xl.py."""
    import subprocess
    import sys
    from pathlib import Path

    tool = Path(__file__).resolve().parent.parent / "tools" / "race_screen_xl.py"
    run = subprocess.run([sys.executable, str(tool), "6"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "race screen: clean" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


def test_colsum_batched_and_linear_fwd_batched(ops):
    """per-image column sums in one pair of launches; eight same-shape projections in one launch (the hoisted key / value
    projections of cross-attention)"""
    import ctypes as C

    from neurosis_amd.lib import call, query

    nb, M, N = 4, 1000, 320
    dy = rnd(nb * M, N)
    out = torch.full((nb, N), 5.0, device="cuda")
    ws = torch.empty(nb * query("nk_colsum_ws_floats", M, N), device="cuda")
    call("nk_colsum_batched", dev(dy).data_ptr(), out.data_ptr(), ws.data_ptr(), M, N, N, nb, 0, ops._stream())
    assert_close(out, dy.view(nb, M, N).sum(1), TOL_F32, "colsum_batched")
    x = rnd(308, 2048)
    ws_ = [rnd(2560, 2048, scale=2048 ** -0.5, seed=i) for i in range(11)]      # 8 + 3: two launches
    outs = ops.gemm_nt_batched([dev(x)] * 11, [dev(w) for w in ws_])
    for w, o in zip(ws_, outs):
        assert_close(o, x @ w.t(), TOL_BF16, "linear_fwd_batched")


@pytest.mark.parametrize("shape", [(4096, 5120, 1280), (16384, 2560, 640), (1000, 384, 256)])
def test_feedforward_projection_with_fused_geglu_forward(ops, shape, monkeypatch):
    """FeedForward.net[0] (modules/attention.py:50-57): the GEGLU in the projection's epilogue (nk_linear_fwd_geglu, the two SDXL widths at batch 4)
    gives bit for bit what the projection followed by the GEGLU kernel gives -- u, the saved pre-activation, and h -- and both agree with torch;
    a shape the 256 x 256 kernel does not take (the third) falls back to the two launches behind the same call."""
    import torch.nn.functional as F

    from neurosis_amd.lib import query

    M, I, K = shape
    x, w = rnd(M, K), rnd(2 * I, K, scale=K ** -0.5)
    b = torch.randn(2 * I, generator=torch.Generator().manual_seed(9)) * 0.1
    wp = torch.nn.Parameter(w.float().cuda())
    bp = torch.nn.Parameter(b.cuda())
    fused = bool(query("nk_linear_fwd_geglu_ok", M, I, K))
    assert fused is (M >= 4096)
    # bit for bit with every XCD walking k from 0: under the default rotated order (NK_GEMM_KROT, gemm_g2.h OpG2::rotate) the k-slabs of an output
    # element are summed in an order that depends on the XCD its tile lands on, and the fused kernel's column tiles are not the plain one's
    monkeypatch.setenv("NK_GEMM_KROT", "0")
    from neurosis_amd import lib

    lib.launch_log(1)
    u, h, bwd = ops.linear_geglu_fwd(dev(x), wp, bp)
    names = lib.launched()
    lib.launch_log(0)
    if fused:     # the library's own word for what ran, not this test's belief (tests/gemm_exact.py)
        assert "nk_gemm_xl2g_kernel<geglu=1>" in names, f"the dispatch moved: the fused GEGLU forward ran {names}; this test needs a shape the kernel takes"
    u2, _ = ops.linear_fwd(dev(x), wp, bp)
    h2 = ops.geglu_fwd(u2)[0]
    assert torch.equal(u, u2) and torch.equal(h, h2)
    monkeypatch.delenv("NK_GEMM_KROT")
    # NOTE: with NK_GEMM_KROT=0 above only the UNROTATED order is compared bit for bit.  The DEFAULT (rotated) order -- what the
    # training step runs -- is checked against the oracle / torch at TOLERANCE only (here and in every parity test), plus the run-to-run stability
    # screen of tools/race_screen_xl.py: two kernels with different tile maps legitimately differ in the last bits under it.
    u, h, bwd = ops.linear_geglu_fwd(dev(x), wp, bp)          # the default order: same values up to the summation order
    assert_close(u, u2.float().cpu(), 1e-2, "geglu projection u, rotated k order")
    assert torch.equal(h, ops.geglu_fwd(u)[0])
    ur = F.linear(x.float(), w.float(), b)
    assert_close(u, ur, 2e-2, "geglu projection u")
    uq = u.float().cpu()
    assert_close(h, uq[:, :I] * F.gelu(uq[:, I:]), 2e-2, "geglu h")
    # the backward closure is the projection's: weight / bias / input gradients of du
    du = rnd(M, 2 * I, seed=5)
    dx = bwd(dev(du))
    ops.join_wgrad_stream()
    assert_close(dx, du.float() @ w.float(), 2e-2, "geglu projection dx")
    assert_close(wp.grad, du.float().t() @ x.float(), 1e-2, "geglu projection dw")
    assert_close(bp.grad, du.float().sum(0), 1e-2, "geglu projection db")
