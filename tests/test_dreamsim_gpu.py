"""DreamSim on the GPU: the new kernels element by element, the towers against the fixture the reference produced in float64
(tests/golden/make_golden_dreamsim.py), one real-width block, and one AutoencodingEngine step with AutoencoderDreamsim.

Bounds.  Kernels that only move or scale data are exact.  The head is fp32: 1e-5 relative to a float64 restatement.  A tower runs the block
code of the CLIP text towers and is held to their bound (tests/test_text_encoder_gpu.py::_close: rel <= 3e-2, cosine >= 0.999).  At the loss
level, d and d / d recons are held to 4 x the deviation the reference's own bf16-autocast run shows for that case (the towers keep their
residual stream in fp32, as autocast does; GEMM, LayerNorm and attention outputs are bf16, and so is the whole backward)."""
from functools import lru_cache, partial

import pytest
import torch
import torch.nn.functional as F

from tests import dreamsim_reference as R
from tests.dreamsim_fixture import checked_state
from tests.golden.fixture_io import load_fixture
from tests.util import cosine, rel_err

pytestmark = pytest.mark.gpu

AUTOCAST_MARGIN = 4.0
DINO, CLIP = R.DINO_NORM, R.CLIP_NORM


def _close(got, want, tol=3e-2):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert rel_err(got, want) <= tol, rel_err(got, want)
    assert cosine(got, want) >= 0.999, cosine(got, want)


@lru_cache(maxsize=None)
def fixture():
    return load_fixture("dreamsim_tiny")


@lru_cache(maxsize=None)
def ensemble():
    from neurosis_amd.modules.losses.dreamsim import DreamsimEnsemble

    fx = fixture()
    ens = DreamsimEnsemble(num_classes=tuple(fx["num_classes"]), vit_config=fx["vit_config"])
    ens.load_state_dict(checked_state(fx))
    return ens.cuda()


def _image(size, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.3 * (torch.rand(3, 3, size, size, generator=g) * 2 - 1)).cuda()          # about a quarter of the pixels outside [-1, 1]


def _rescaled_affine(stats):
    from neurosis_amd import ops

    mean, std = stats
    scale, shift = [0.5 / s for s in std], [(0.5 - m) / s for m, s in zip(mean, std)]
    return ops.vit_affine(scale, shift, -1.0, 1.0), torch.tensor(scale).view(1, 3, 1, 1).cuda(), torch.tensor(shift).view(1, 3, 1, 1).cuda()


def _unfold(y, p=16):
    """[N, 3, H, W] -> [N * Np, 3 p p]: row (n, py, px), column (c, ky, kx)"""
    return F.unfold(y, kernel_size=p, stride=p).transpose(1, 2).reshape(-1, 3 * p * p)


@pytest.mark.parametrize("size", [32, 48])
@pytest.mark.parametrize("stats", [DINO, CLIP], ids=["dino", "clip"])
def test_patchify_is_the_bf16_rounding_of_the_fp32_formula(size, stats):
    from neurosis_amd import ops

    x = _image(size, 11 + size)
    affine, a, b = _rescaled_affine(stats)
    got = ops.vit_patchify(x, 16, affine)
    assert got.shape == (3 * (size // 16) ** 2, 768) and got.dtype == torch.bfloat16
    want = _unfold(a * x.clamp(-1.0, 1.0) + b).to(torch.bfloat16)                       # one fp32 product, one fp32 sum, one rounding
    assert torch.equal(got, want)
    # and that is, to one bf16 step, Normalize(mean, std) of clamp(x / 2 + 0.5, 0, 1): what the reference computes
    mean, std = (torch.tensor(s).view(1, 3, 1, 1).cuda() for s in stats)
    chain = _unfold(((x / 2 + 0.5).clamp(0.0, 1.0) - mean) / std)
    assert float((got.float() - chain).abs().max()) <= 2.0 ** -8 * float(chain.abs().max())
    # without the rescale: plain Normalize, no clamp
    plain = ops.vit_patchify(x, 16, ops.vit_affine([1.0 / s for s in stats[1]], [-m / s for m, s in zip(*stats)]))
    a1, b1 = (torch.tensor(v).view(1, 3, 1, 1).cuda() for v in ([1.0 / s for s in stats[1]], [-m / s for m, s in zip(*stats)]))
    assert torch.equal(plain, _unfold(a1 * x + b1).to(torch.bfloat16))
    with pytest.raises(ValueError, match="multiples of the patch size"):
        ops.vit_patchify(x[:, :, :24].contiguous(), 16, affine)


@pytest.mark.parametrize("size", [32, 48])
def test_patchify_adjoint(size):
    from neurosis_amd import ops

    g = torch.Generator().manual_seed(size)
    # P x = a_c x with a_c a power of two and x, y on the bf16 grid: P x and P^T y are exact, the two inner products differ by fp32 accumulation only
    x = torch.randn(3, 3, size, size, generator=g).to(torch.bfloat16).float().cuda()
    y = torch.randn(3 * (size // 16) ** 2, 768, generator=g).to(torch.bfloat16).cuda()
    lin = ops.vit_affine((0.5, 2.0, 1.0), (0.0, 0.0, 0.0))
    px, pty = ops.vit_patchify(x, 16, lin), ops.vit_patchify_bwd(y, x, 16, lin)
    assert pty.shape == x.shape and pty.dtype == torch.float32
    lhs, rhs = float((px.double() * y.double()).sum()), float((x.double() * pty.double()).sum())
    scale = float((px.double() * y.double()).abs().sum())
    assert abs(lhs - rhs) <= 1e-6 * scale, (lhs, rhs)
    # with the clamp: a_c y inside [-1, 1], zero where the forward clamped (about a third of these pixels)
    affine, a, _ = _rescaled_affine(CLIP)
    wide = 1.5 * x
    got = ops.vit_patchify_bwd(y, wide, 16, affine)
    folded = F.fold(y.float().reshape(3, -1, 768).transpose(1, 2), (size, size), kernel_size=16, stride=16)
    inside = (wide >= -1.0) & (wide <= 1.0)
    assert 0.2 < float((~inside).float().mean()) < 0.6
    assert torch.equal(got, a * folded * inside)
    # accumulate: the sum, and two runs give equal bits
    base = torch.randn(x.shape, generator=g).cuda()
    r1 = ops.vit_patchify_bwd(y, wide, 16, affine, out=base.clone())
    r2 = ops.vit_patchify_bwd(y, wide, 16, affine, out=base.clone())
    assert torch.equal(r1, r2)
    assert float((r1 - (base + got)).abs().max()) <= 1e-6 * float((base.abs() + got.abs()).max())


def test_token_assembly_and_its_adjoint():
    from neurosis_amd import ops

    g = torch.Generator().manual_seed(3)
    N, Np, E = 3, 9, 128
    patches = torch.randn(N * Np, E, generator=g).to(torch.bfloat16).cuda()
    cls, pos = torch.randn(E, generator=g).cuda(), torch.randn(Np + 1, E, generator=g).cuda()
    got = ops.vit_tokens(patches, cls, pos, N)
    want = (torch.cat((cls.expand(N, 1, E), patches.float().view(N, Np, E)), dim=1) + pos).view(N * (Np + 1), E)      # the stream is fp32
    assert got.dtype == torch.float32 and torch.equal(got, want)
    d = torch.randn(N * (Np + 1), E, generator=g).to(torch.bfloat16).cuda()
    assert torch.equal(ops.vit_tokens_bwd(d, N), d.view(N, Np + 1, E)[:, 1:].reshape(N * Np, E))


@pytest.mark.parametrize("M,E", [(10, 128), (7, 768), (5, 200)])
def test_fp32_stream_seam_add_and_layernorm(M, E):
    from neurosis_amd import ops

    g = torch.Generator().manual_seed(M * E)
    x = (1.5 * torch.randn(M, E, generator=g) + 0.2).cuda()
    branch = torch.randn(M, E, generator=g).to(torch.bfloat16).cuda()
    norm = torch.nn.LayerNorm(E, eps=1e-6)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.2 * torch.randn(E, generator=g))
        norm.bias.copy_(0.2 * torch.randn(E, generator=g))
    norm = norm.cuda().requires_grad_(False)
    summed = x + branch.float()                                                          # one fp32 add: exact to compare
    want = F.layer_norm(summed.double(), (E,), norm.weight.double(), norm.bias.double(), 1e-6)
    stream = x.clone()
    y, xb, mean, rstd = ops.vit_add_ln(stream, branch, norm, copy=True)
    assert torch.equal(stream, summed) and torch.equal(xb, summed.to(torch.bfloat16)) and y.dtype == torch.bfloat16
    assert float((y.double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())      # half a bf16 step of the largest entry
    assert rel_err(mean, summed.double().mean(dim=1)) <= 1e-5
    assert rel_err(rstd, (summed.double().var(dim=1, unbiased=False) + 1e-6).rsqrt()) <= 1e-5
    # fp32 output (norm_pre), no branch: x untouched
    stream = x.clone()
    y32, none, _, _ = ops.vit_add_ln(stream, None, norm, y_f32=True)
    assert none is None and torch.equal(stream, x) and y32.dtype == torch.float32
    assert rel_err(y32, F.layer_norm(x.double(), (E,), norm.weight.double(), norm.bias.double(), 1e-6)) <= 1e-5
    # the add alone
    stream = x.clone()
    assert ops.vit_add_ln(stream, branch, None)[0] is None and torch.equal(stream, summed)


@pytest.mark.parametrize("with_norm,with_head", [(True, True), (False, False), (True, False)])
def test_cls_row_final_norm_and_head_in_fp32(with_norm, with_head):
    from neurosis_amd import ops

    g = torch.Generator().manual_seed(17)
    N, L, E, nc, s = 4, 5, 128, 24, 2
    tokens = (2.0 * torch.randn(N * L, E, generator=g) + 0.3).cuda()
    norm = torch.nn.LayerNorm(E, eps=1e-5) if with_norm else None
    head = torch.nn.Linear(E, nc) if with_head else None
    with torch.no_grad():
        for p in [q for m in (norm, head) if m is not None for q in m.parameters()]:
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() == 1 else E ** -0.5) + (1.0 if p.dim() == 1 else 0.0))
    for m in (norm, head):
        if m is not None:
            m.cuda().requires_grad_(False)
    out, bwd = ops.vit_cls_head(tokens, N, norm, head, tape_from=s)
    dout = torch.randn(N - s, out.shape[1], generator=g).cuda()
    dcls = bwd(dout)
    rows = tokens.view(N, L, E)[:, 0].double().cpu().requires_grad_(True)
    want = rows
    if with_norm:
        want = F.layer_norm(want, (E,), norm.weight.double().cpu(), norm.bias.double().cpu(), 1e-5)
    if with_head:
        want = F.linear(want, head.weight.double().cpu(), head.bias.double().cpu())
    (dwant,) = torch.autograd.grad(want[s:], rows, dout.double().cpu())
    assert out.dtype == torch.float32 and out.shape == want.shape and rel_err(out, want.detach()) <= 1e-5
    # the gradient leaves as bf16 (it joins the bf16 token gradient): half a bf16 step of its largest entry
    assert dcls.shape == (N - s, E) and rel_err(dcls, dwant[s:]) <= 2.0 ** -8
    assert torch.equal(ops.vit_cls_head(tokens, N, norm, head)[0], out)


def _head64(f, up):
    f = f.double().cpu().requires_grad_(True)
    z = f / f.norm(dim=-1, keepdim=True)
    z = z - z.mean(dim=-1, keepdim=True)
    d = 1 - F.cosine_similarity(z[0], z[1], dim=1, eps=1e-8)
    (g,) = torch.autograd.grad((d * up.double().cpu()).sum(), f)
    return d.detach(), g[1], g[0]


@pytest.mark.parametrize("B,Dz,noise", [(3, 160, 0.3), (2, 1792, 0.3), (3, 160, 5.0), (2, 1792, 5.0)])
def test_head_against_float64(B, Dz, noise):
    from neurosis_amd import ops

    g = torch.Generator().manual_seed(B * Dz)
    f0 = torch.randn(B, Dz, generator=g) + 0.5                                          # a mean for the centring to remove
    f = torch.stack((f0, f0 + noise * torch.randn(B, Dz, generator=g))).cuda()
    up = torch.randn(B, generator=g).cuda()
    d, bwd = ops.dreamsim_head(f)
    df1 = bwd(up)
    d64, g64, _ = _head64(f, up)
    print(f"head B={B} Dz={Dz}: d {d64.tolist()}; d err {rel_err(d, d64):.2e}, df1 err {rel_err(df1, g64):.2e}")
    assert float((d.cpu().double() - d64).abs().div(d64.abs()).max()) <= 1e-5             # each d_b, relative to itself
    assert rel_err(df1, g64) <= 1e-5 and df1.shape == (B, Dz)
    d2, bwd2 = ops.dreamsim_head(f)
    assert torch.equal(d, d2) and torch.equal(df1, bwd2(up))                              # fixed-order sums


def _loss_level(size):
    """(d, d sum(d) / d recons, per-tower embeddings) of the tiny ensemble on the fixture's images, rescale_input on"""
    case = fixture()["cases"][str(size)]
    ens = ensemble()
    x, recons = case["inputs"].cuda().clamp(-1.0, 1.0), case["recons"].cuda()
    d, bwd = ens.fwdb(x, recons, rescale=True)
    grad = bwd(torch.ones(3, device="cuda"))
    both = torch.cat((x, recons)).contiguous()
    emb = {name: tower.features(both, affine, norm=norm)[0] for (tower, affine, norm), name in zip(ens._towers(True, True), ("dino", "clip1", "clip2"))}
    return case, d, grad, emb


@pytest.mark.parametrize("size", [32, 48])
def test_towers_and_loss_against_the_reference_fixture(size):
    """Per-tower embeddings inside the CLIP towers' bound; d and d(sum d) / d recons inside 4 x the reference's own bf16-autocast deviation.
    Measured on an MI355X: embeddings 8.1e-3 .. 1.3e-2; d 5.13e-3 = 1.14 x autocast at 32 and 5.46e-3 = 0.51 x at 48; gradient
    2.21e-2 = 0.93 x at 32 and 1.78e-2 = 0.97 x at 48.  (With a bf16 residual stream d at 32 was 2.06e-2 = 4.58 x: the stream is fp32 for that.)"""
    case, d, grad, emb = _loss_level(size)
    for name, got in emb.items():
        want, ac = case["emb"][name], case["autocast"]["emb"][name]
        print(f"{size} {name}: embedding err {rel_err(got, want):.3e} cos {cosine(got, want):.6f}   (reference under bf16 autocast: {ac['rel']:.3e} / {ac['cosine']:.6f})")
    for name, got in emb.items():
        _close(got, case["emb"][name])
    ac_d, ac_g = case["autocast"]["d"]["rel"], case["autocast"]["grad"]["rel"]
    err_d, err_g = rel_err(d, case["d"]), rel_err(grad, case["grad"])
    print(f"{size}: d {d.tolist()} / {case['d'].tolist()}")
    print(f"{size}: d err {err_d:.3e} = {err_d / ac_d:.2f} x autocast ({ac_d:.3e});  grad err {err_g:.3e} = {err_g / ac_g:.2f} x autocast ({ac_g:.3e}), "
          f"cos {cosine(grad, case['grad']):.6f}")
    assert grad.shape == case["grad"].shape and grad.dtype == torch.float32
    assert err_d <= AUTOCAST_MARGIN * ac_d
    assert err_g <= AUTOCAST_MARGIN * ac_g
    # forward() is the same distance without a tape
    x, recons = case["inputs"].cuda().clamp(-1.0, 1.0), case["recons"].cuda()
    d01 = ensemble()(torch.stack(((x / 2 + 0.5).clamp(0, 1), (recons / 2 + 0.5).clamp(0, 1))))
    assert rel_err(d01, case["d"]) <= AUTOCAST_MARGIN * ac_d
    assert all(p.grad is None for p in ensemble().parameters())


def test_fwdb_is_reproducible_and_resizes():
    from neurosis_amd.modules.losses.dreamsim import DreamsimEnsemble

    fx = fixture()
    case = fx["cases"]["48"]
    x, recons = case["inputs"].cuda().clamp(-1.0, 1.0), case["recons"].cuda()
    up = torch.tensor([1.0, 0.0, -2.0], device="cuda")
    runs = []
    for _ in range(2):
        d, bwd = ensemble().fwdb(x, recons, rescale=True)
        runs.append((d, bwd(up)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1][1].abs().max()) == 0.0                                      # upstream 0: that sample's image gets no gradient
    # do_resize: 48 x 48 images through the 32 x 32 towers; the gradient comes back at 48 x 48, and is the one of the resized images pulled back
    small = DreamsimEnsemble(image_size=32, do_resize=True, num_classes=tuple(fx["num_classes"]), vit_config=fx["vit_config"])
    small.load_state_dict(checked_state(fx))
    small = small.cuda()
    d, bwd = small.fwdb(x, recons, rescale=True)
    g = bwd(torch.ones(3, device="cuda"))
    # the same function evaluated the other way round: resize first (F.interpolate), map to [0, 1], and ask the un-resizing model; its gradient
    # w.r.t. the [0, 1] images is halved by the rescale and pulled back by the resize's adjoint.  Both are bf16 evaluations of one function,
    # each within the loss-level bound of this case, so they differ by at most twice that.
    from neurosis_amd import ops

    xs, rs = (F.interpolate(t, size=(32, 32), mode="bicubic", antialias=True) / 2 + 0.5 for t in (x, recons))
    d_want, bwd_want = ensemble().fwdb(xs.contiguous(), rs.contiguous(), rescale=False)
    g_want = ops.resize_bicubic_aa_bwd((0.5 * bwd_want(torch.ones(3, device="cuda"))).contiguous(), (48, 48))
    assert g.shape == recons.shape and g.dtype == torch.float32
    print(f"do_resize: d {rel_err(d, d_want):.3e}, gradient {rel_err(g, g_want):.3e} cos {cosine(g, g_want):.6f}")
    assert rel_err(d, d_want) <= 2 * AUTOCAST_MARGIN * case["autocast"]["d"]["rel"]
    assert rel_err(g, g_want) <= 2 * AUTOCAST_MARGIN * case["autocast"]["grad"]["rel"]


@pytest.mark.parametrize("L,quick", [(197, False), (257, True)])
def test_one_real_width_block_forward_and_input_gradient(L, quick):
    from neurosis_amd import lib
    from neurosis_amd.modules.losses.dreamsim import vit as V

    E, heads, N = 768, 12, 2
    g = torch.Generator().manual_seed(L)
    blk = V.Block(E, heads, 4.0, True, partial(torch.nn.LayerNorm, eps=1e-6))
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    blk = blk.cuda().requires_grad_(False)
    x = torch.randn(N * L, E, generator=g).cuda()
    dy = torch.randn(N * L, E, generator=g).to(torch.bfloat16).cuda()
    y = x.clone()
    tape = V._block_forward(y, blk, N, quick, 0)                                          # the fp32 stream, updated in place
    assert y.dtype == torch.float32
    lib.launch_log(1)
    try:
        dx = V._block_backward(dy, blk, tape, N, quick)
        log = lib.launched()
    finally:
        lib.launch_log(0)
    # the fp32 restatement
    xr = x.view(N, L, E).clone().requires_grad_(True)
    h = F.layer_norm(xr, (E,), blk.norm1.weight, blk.norm1.bias, 1e-6)
    qkv = F.linear(h, blk.attn.qkv.weight, blk.attn.qkv.bias).reshape(N, L, 3, heads, E // heads).permute(2, 0, 3, 1, 4)
    t = xr + F.linear(F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(N, L, E), blk.attn.proj.weight, blk.attn.proj.bias)
    u = F.linear(F.layer_norm(t, (E,), blk.norm2.weight, blk.norm2.bias, 1e-6), blk.mlp.fc1.weight, blk.mlp.fc1.bias)
    want = t + F.linear(u * torch.sigmoid(1.702 * u) if quick else F.gelu(u), blk.mlp.fc2.weight, blk.mlp.fc2.bias)
    (dwant,) = torch.autograd.grad(want, xr, dy.float().view(N, L, E))
    print(f"L={L}: forward err {rel_err(y, want.reshape(N * L, E)):.3e}, input gradient err {rel_err(dx, dwant.reshape(N * L, E)):.3e} "
          f"cos {cosine(dx, dwant.reshape(N * L, E)):.6f}")
    _close(y.float(), want.detach().reshape(N * L, E))
    _close(dx.float(), dwant.reshape(N * L, E))
    # input gradients only: no weight-gradient, column-sum or LayerNorm-parameter kernel among the launches
    names = " ".join(log)
    assert "ln_bwd_dx_kernel" in names, log
    assert not any(s in names for s in ("wgrad", "colpart", "colsum", "ln_bwd_rows", "ln_bwd_param")), log
    assert all(p.grad is None for p in blk.parameters())


@lru_cache(maxsize=None)
def _engine_case():
    import json

    from tests.golden.fixture_io import HERE as G
    from tests.golden.make_golden import synth_state_dict

    fx = load_fixture("vae_train_tiny")
    return fx["cfg"], synth_state_dict(json.loads((G / "vae_train_tiny_keys.json").read_text())), fx["x"], fx["cases"]["rec_only"]["noise"]


@pytest.mark.parametrize("rec_type", ["l1", "l2"])
def test_engine_step_with_autoencoder_dreamsim(rec_type):
    from neurosis_amd import ops
    from neurosis_amd.models.autoencoder import AutoencodingEngine, DiagonalGaussianRegularizer
    from neurosis_amd.modules.autoencoding.losses import AutoencoderDreamsim
    from neurosis_amd.modules.diffusion.model import Decoder, Encoder

    REC_W, DS_W = 0.6, 0.8
    fx = fixture()
    cfg, sd, x, noise = _engine_case()
    loss = AutoencoderDreamsim(dreamsim_weight=DS_W, recon_type=rec_type, recon_weight=REC_W, vit_config={**fx["vit_config"], "num_classes": fx["num_classes"][1]})
    weights = checked_state(fx)
    loss.dreamsim_loss.load_state_dict(weights)
    eng = AutoencodingEngine(encoder=Encoder(**cfg), decoder=Decoder(**cfg), loss=loss, regularizer=DiagonalGaussianRegularizer(sample=True))
    eng.encoder.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")})
    eng.decoder.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")})
    eng = eng.cuda().train()
    eng.setup_flat_params()
    assert eng.perceptual_only and eng.discriminator is None and eng.disc_store is None
    x = x.cuda()
    total, _, xrec, log = eng.loss_and_backward(x, noise=noise.cuda())
    for key in ("loss/total", "loss/rec", "loss/p"):
        assert log[key].is_cuda and log[key].dim() == 0 and not log[key].requires_grad
    assert abs(float(total) - float(log["loss/rec"]) - float(log["loss/p"])) <= 1e-6 * abs(float(total)) and float(total) == float(log["loss/total"])
    assert float(log["loss/p"]) > 0
    assert all(p.grad is None for p in eng.loss.dreamsim_loss.parameters())              # frozen towers collect no weight gradients
    assert float(eng.store.grad.abs().max()) > 0

    # the gradient at the decoder's output, against CPU autograd through the restatement fed the GPU's reconstruction
    B, C, H, W = xrec.shape
    _, d_tokens, _ = eng._perceptual_loss(x, xrec, ops.Img(ops.nchw_to_tokens(xrec, 8), B, H, W))
    got = ops.tokens_to_nchw(d_tokens, B, C, H, W)
    heads = fx["vit_config"]["num_heads"]
    sd64 = {k: v.double() for k, v in weights.items()}
    r64 = xrec.double().cpu().requires_grad_(True)
    want_loss, want_rec, want_p = R.autoencoder_dreamsim(sd64, x.double().cpu(), r64, heads, rec_type, REC_W, DS_W)
    (want,) = torch.autograd.grad(want_loss, r64)
    # what bf16 autocast costs the same restatement on this case: the loss-level yardstick
    r32 = xrec.cpu().clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        ac_loss, _, ac_p = R.autoencoder_dreamsim(weights, x.cpu(), r32, heads, rec_type, REC_W, DS_W)
    (ac,) = torch.autograd.grad(ac_loss, r32)
    ac_g, ac_p_rel = rel_err(ac, want), abs(float(ac_p.detach()) - float(want_p.detach())) / float(want_p.detach())
    err_g, err_p = rel_err(got, want), abs(float(log["loss/p"]) - float(want_p.detach())) / float(want_p.detach())
    clamped = float(((xrec < -1) | (xrec > 1)).float().mean())
    print(f"{rec_type}: loss {float(total):.6f} / {float(want_loss.detach()):.6f}; p err {err_p:.3e} = {err_p / ac_p_rel:.2f} x autocast ({ac_p_rel:.3e}); "
          f"gradient err {err_g:.3e} = {err_g / ac_g:.2f} x autocast ({ac_g:.3e}), cos {cosine(got, want):.6f}; clamped share {clamped:.3f}")
    assert abs(float(log["loss/rec"]) - float(want_rec.detach().mean())) <= 1e-5 * float(want_rec.detach().mean())
    assert err_p <= AUTOCAST_MARGIN * ac_p_rel
    assert err_g <= AUTOCAST_MARGIN * ac_g
    assert float(got[(xrec < -1) | (xrec > 1)].abs().max() if clamped > 0 else 0.0) == 0.0   # no gradient where xrec was clamped
