"""Dropout on the GPU: nk_dropout bit for bit against the CPU restatement (tests/dropout_ref.py), tokens and the counter, the four module
sites against float64 with the restated mask, neutrality at rate 0 / in eval mode, hipGraph replay and the engine's micro-batches.

Float64 bounds are the project's own for these modules without dropout: output and input gradients rel_err <= 3e-2 and cosine >= 0.999
(test_modules_gpu.py::test_public_module_forward_autograd_vs_oracle), parameter gradients check_grad_cosines's floors 0.999 / 0.99.  Every
float64 comparison has a negative control: against the reference evaluated with the mask of ANOTHER step the output error must exceed 3e-2,
or the comparison could not see a wrong mask."""
import json
import os
from pathlib import Path

import pytest
import torch

from tests import dropout_ref as R
from tests.util import bf16_round, check_grad_cosines, cosine, rel_err

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
BF = torch.bfloat16
P = 0.25


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int16).cpu()


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _randn_bf16(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(BF)


# ------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows, cols", [(1, 8), (3, 40), (257, 320)])
def test_kernel_equals_the_restatement_bit_for_bit(rows, cols, p):
    from neurosis_amd import ops

    seed, site = 1234, 7
    ops.dropout_seed(seed, 2)
    ops.dropout_draw()                                           # step 3
    assert ops.dropout_state() == (seed, 3)
    keep = R.keep_mask(rows, cols, p, seed, 3, site)
    x, r, dy = (_randn_bf16(rows, cols, seed=s) for s in (1, 2, 3))
    x[0, :3] = torch.tensor([float("inf"), -0.0, 0.0], dtype=BF)
    dropped = (~keep[0]).nonzero().flatten().tolist()
    if dropped:
        x[0, dropped[0]] = float("nan")                          # a dropped element is +0 whatever it held: a select, not a product
    for residual in (None, r):
        want = R.apply_exact(x, keep, p, residual)
        for inplace in (False, True):
            xg = x.cuda()
            y, bwd = ops.dropout_fwd(xg, p, site, residual=None if residual is None else residual.cuda(), inplace=inplace)
            assert (y.data_ptr() == xg.data_ptr()) == inplace
            assert _same_bits(y, want), (rows, cols, p, residual is not None, inplace)
            if not inplace:
                assert _same_bits(xg, x)
            dyg = dy.cuda()
            dx = bwd(dyg, inplace=inplace)
            assert (dx.data_ptr() == dyg.data_ptr()) == inplace
            assert _same_bits(dx, R.apply_exact(dy, keep, p))
    assert ops.dropout_state() == (seed, 3)                      # masks and backwards do not draw


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_one_mask_over_both_column_halves_of_a_wider_buffer(p):
    """[64, 2560] laid over each half of a [64, 5120] buffer (row stride 5120): the mask goes by the logical index, not the stride"""
    from neurosis_amd import ops

    seed, site, M, I = 99, 11, 64, 2560
    ops.dropout_seed(seed, 0)
    tok = ops.dropout_draw()
    keep = R.keep_mask(M, I, p, seed, 1, site)
    buf = _randn_bf16(M, 2 * I, seed=4)
    g = buf.cuda()
    ops.dropout_mask_like(g[:, :I], p, site, tok)
    ops.dropout_mask_like(g[:, I:], p, site, tok)
    assert _same_bits(g[:, :I], R.apply_exact(buf[:, :I], keep, p)) and _same_bits(g[:, I:], R.apply_exact(buf[:, I:], keep, p))
    out = ops.dropout_mask_like(buf.cuda()[:, I:], p, site, tok, inplace=False)          # strided in, dense out
    assert out.is_contiguous() and _same_bits(out, R.apply_exact(buf[:, I:], keep, p))
    import neurosis_amd.torch_ops  # noqa: F401  (registers torch.ops.neurosis_hip.*)

    y = torch.ops.neurosis_hip.dropout(buf.cuda()[:, :I], tok, p, site)
    assert _same_bits(y, R.apply_exact(buf[:, :I], keep, p))
    with pytest.raises(ValueError):
        ops.dropout_mask_like(buf.cuda()[:, :36], p, site, tok)                           # cols % 8
    with pytest.raises(ValueError):
        ops.dropout_mask_like(buf.cuda()[:, 4:12], p, site, tok)                          # rows not 16-byte aligned


# ------------------------------------------------------------------------------------------------
# 2. tokens
# ------------------------------------------------------------------------------------------------
def test_tokens_bind_the_mask_of_their_own_forward():
    from neurosis_amd import ops

    x1, x2, dy = (_randn_bf16(33, 64, seed=s).cuda() + 4.0 for s in (5, 6, 7))         # (+ 4: no input zeros, so the zeros ARE the mask)

    def calls():
        t1 = ops.dropout_draw()
        y1, b1 = ops.dropout_fwd(x1, 0.5, 3)
        y1_again, _ = ops.dropout_fwd(x1, 0.5, 3)
        t2 = ops.dropout_draw()
        y2, b2 = ops.dropout_fwd(x2, 0.5, 3)                       # interleaved: the second forward before the first backward
        d1, d2 = b1(dy), b2(dy)
        return t1.cpu(), t2.cpu(), y1, y1_again, y2, d1, d2

    ops.dropout_seed(77, 5)
    t1, t2, y1, y1_again, y2, d1, d2 = calls()
    assert t1.tolist() == [77, 6] and t2.tolist() == [77, 7] and ops.dropout_state() == (77, 7)
    assert _same_bits(y1, y1_again)                                # one token used twice: equal bits
    z1, z2 = (y1 == 0), (y2 == 0)
    assert not torch.equal(z1, z2) and 0.3 < float(z1.double().mean()) < 0.7
    assert torch.equal(z1.cpu(), ~R.keep_mask(33, 64, 0.5, 77, 6, 3)) and torch.equal(z2.cpu(), ~R.keep_mask(33, 64, 0.5, 77, 7, 3))
    assert torch.equal(d1 == 0, z1) and torch.equal(d2 == 0, z2)   # each backward regenerates the mask of ITS forward
    ops.dropout_seed(77, 5)
    again = calls()
    assert again[0].tolist() == [77, 6]
    for a, b in zip((y1, y1_again, y2, d1, d2), again[2:]):
        assert _same_bits(a, b)                                    # dropout_seed(s, k) + the same calls: every bit again
    big = (1 << 63) + 12345                                        # a seed that uses the high key word and the sign bit of the int64 storage
    ops.dropout_seed(big, (1 << 32) + 1)
    ops.dropout_draw()
    assert ops.dropout_state() == (big, (1 << 32) + 2)
    y, _ = ops.dropout_fwd(x1, 0.5, 3)
    assert torch.equal((y == 0).cpu(), ~R.keep_mask(33, 64, 0.5, big, (1 << 32) + 2, 3))


# ------------------------------------------------------------------------------------------------
# float64 helpers
# ------------------------------------------------------------------------------------------------
def _randomize(mod, seed):
    torch.manual_seed(seed)
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if p.dim() == 1:
                v = torch.randn(p.shape) * 0.5 + (1.0 if k.endswith("weight") else 0.0)     # (1-D weights are norm scales)
            else:
                v = torch.randn(p.shape) * p[0].numel() ** -0.5                             # (also the zero-initialised output convolution)
            p.copy_(bf16_round(v))
    return mod


def _sd64(mod, prefix):
    return {f"{prefix}.{k}": v.detach().double().cpu().contiguous().clone().requires_grad_(True) for k, v in mod.state_dict().items()}


def _against_float64(label, got_out, ref_out, wrong_out, got_in, ref_in, got_grads, ref_grads):
    """the bounds of the module docstring; prints every figure before it asserts"""
    e, neg = rel_err(got_out, ref_out), rel_err(got_out, wrong_out)
    ins = [(rel_err(g, r), cosine(g, r)) for g, r in zip(got_in, ref_in)]
    print(f"[dropout fp64] {label}: out rel_err {e:.3e} (another step's mask: {neg:.3e}); input grads {[(round(a, 5), round(c, 6)) for a, c in ins]}")
    check_grad_cosines(f"dropout {label}", got_grads, ref_grads)
    assert e <= 3e-2
    for a, c in ins:
        assert a <= 3e-2 and c >= 0.999
    assert neg > 3e-2, "the comparison cannot see a wrong mask"


# ------------------------------------------------------------------------------------------------
# 3. ResBlock
# ------------------------------------------------------------------------------------------------
RB_N, RB_H, RB_W = 2, 8, 8


def _resblock(p=P, **kw):
    from neurosis_amd.modules.diffusion.openaimodel import ResBlock

    return _randomize(ResBlock(64, 128, p, out_channels=96, **kw), 3)


def _rb_inputs(seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return (bf16_round(torch.randn(RB_N, 64, RB_H, RB_W, generator=g)), bf16_round(torch.randn(RB_N, 128, generator=g)),
            bf16_round(torch.randn(RB_N, 96, RB_H, RB_W, generator=g)))


def _rb_mult(seed, step, site=0):
    return R.tokens_to_nchw(R.multiplier(RB_N * RB_H * RB_W, 96, P, seed, step, site), RB_N, RB_H, RB_W)


def _rb_run(rb, x, emb, dy):
    xg, eg = x.cuda().requires_grad_(True), emb.cuda().requires_grad_(True)
    out = rb(xg, eg)
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    return out.detach().clone(), xg.grad.clone(), eg.grad.clone(), {k: p.grad.clone() for k, p in rb.named_parameters()}


def test_resblock_against_float64():
    from neurosis_amd import ops

    rb = _resblock()
    sd = _sd64(rb, "b")
    x, emb, dy = _rb_inputs()
    xr, er = x.double().requires_grad_(True), emb.double().requires_grad_(True)
    ref = R.resblock(sd, "b", xr, er, _rb_mult(11, 1))
    ref.backward(dy.double())
    with torch.no_grad():
        wrong = R.resblock(sd, "b", xr, er, _rb_mult(11, 2))
    rb = rb.cuda()
    ops.dropout_seed(11, 0)
    out, dx, demb, grads = _rb_run(rb, x, emb, dy)
    assert ops.dropout_state() == (11, 1)                          # the public forward drew once; the backward did not
    assert float((out.float() == 0).double().mean()) < 0.01       # (the mask sits in front of a convolution: the output itself is dense)
    _against_float64("ResBlock", out, ref, wrong, [dx, demb], [xr.grad, er.grad], grads, {k[2:]: v.grad for k, v in sd.items()})


def test_resblock_use_checkpoint_is_bit_identical():
    """the re-run of _fwd inside the backward sees the token of its own forward, although another draw happened in between"""
    from neurosis_amd import ops

    rb = _resblock().cuda()
    x, emb, dy = _rb_inputs()
    res = []
    for ck in (False, True):
        rb.use_checkpoint = ck
        ops.dropout_seed(11, 0)
        xg, eg = x.cuda().requires_grad_(True), emb.cuda().requires_grad_(True)
        out = rb(xg, eg)
        ops.dropout_draw()                                         # a later draw (another model's forward, say) must not leak into the re-run
        out.backward(dy.cuda())
        torch.cuda.synchronize()
        res.append((out.detach().clone(), xg.grad.clone(), eg.grad.clone(), {k: p.grad.clone() for k, p in rb.named_parameters()}))
    (o0, dx0, de0, g0), (o1, dx1, de1, g1) = res
    assert _same_bits(o0, o1) and torch.equal(dx0, dx1) and torch.equal(de0, de1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_resblock_two_forwards_then_one_backward_of_the_sum():
    from neurosis_amd import ops

    rb = _resblock()
    sd = _sd64(rb, "b")
    (x1, e1, dy), (x2, e2, _) = _rb_inputs(1), _rb_inputs(2)
    leaves = [t.double().requires_grad_(True) for t in (x1, e1, x2, e2)]
    ref = R.resblock(sd, "b", leaves[0], leaves[1], _rb_mult(21, 1)) + R.resblock(sd, "b", leaves[2], leaves[3], _rb_mult(21, 2))
    ref.backward(dy.double())
    with torch.no_grad():                                          # both masks of the step after
        wrong = R.resblock(sd, "b", leaves[0], leaves[1], _rb_mult(21, 2)) + R.resblock(sd, "b", leaves[2], leaves[3], _rb_mult(21, 3))
    rb = rb.cuda()
    for p in rb.parameters():
        p.grad = None
    ops.dropout_seed(21, 0)
    gl = [t.cuda().requires_grad_(True) for t in (x1, e1, x2, e2)]
    ops.state.grad_accumulate = True                               # both backward passes ADD to the (zero-initialised) parameter gradients
    try:
        out = rb(gl[0], gl[1]) + rb(gl[2], gl[3])
        out.backward(dy.cuda())
        torch.cuda.synchronize()
    finally:
        ops.state.grad_accumulate = False
    assert ops.dropout_state() == (21, 2)
    _against_float64("ResBlock, two forwards", out, ref, wrong, [t.grad for t in gl], [t.grad for t in leaves],
                     {k: p.grad for k, p in rb.named_parameters()}, {k[2:]: v.grad for k, v in sd.items()})


# ------------------------------------------------------------------------------------------------
# 4. BasicTransformerBlock (CrossAttention.to_out twice, FeedForward)
# ------------------------------------------------------------------------------------------------
TB_B, TB_L, TB_C, TB_LC, TB_CC = 2, 64, 128, 7, 64


def _tblock(p=P, **kw):
    from neurosis_amd.modules.attention import BasicTransformerBlock

    return _randomize(BasicTransformerBlock(TB_C, 2, 64, dropout=p, context_dim=TB_CC, **kw), 5)


def _tb_inputs():
    g = torch.Generator().manual_seed(200)
    return (bf16_round(torch.randn(TB_B, TB_L, TB_C, generator=g)), bf16_round(torch.randn(TB_B, TB_LC, TB_CC, generator=g)),
            bf16_round(torch.randn(TB_B, TB_L, TB_C, generator=g)))


def _tb_mults(blk, seed, step):
    site = {id(m): i for i, m in enumerate(blk.modules())}
    rows = TB_B * TB_L
    return (R.multiplier(rows, TB_C, P, seed, step, site[id(blk.attn1)]).view(TB_B, TB_L, TB_C),
            R.multiplier(rows, TB_C, P, seed, step, site[id(blk.attn2)]).view(TB_B, TB_L, TB_C),
            R.multiplier(rows, 4 * TB_C, P, seed, step, site[id(blk.ff)]).view(TB_B, TB_L, 4 * TB_C))


def _tb_run(blk, x, ctx, dy):
    xg, cg = x.cuda().requires_grad_(True), ctx.cuda().requires_grad_(True)
    out = blk(xg, cg)
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    return out.detach().clone(), xg.grad.clone(), cg.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}


@pytest.mark.parametrize("form", ["saved_derivative", "geglu_save_0", "recompute_norms"])
def test_transformer_block_against_float64(form, monkeypatch):
    """the three saved forms of the FeedForward: s = [gelu(g) | a gelu'(g)] (default), u = [a | g] (NK_GEGLU_SAVE=0), and u with h rebuilt
    in the backward (recompute = 'norms')"""
    from neurosis_amd import ops

    if form == "geglu_save_0":
        monkeypatch.setenv("NK_GEGLU_SAVE", "0")
    blk = _tblock(checkpoint=False)
    if form == "recompute_norms":
        blk.recompute = "norms"
    sd = _sd64(blk, "t")
    x, ctx, dy = _tb_inputs()
    xr, cr = x.double().requires_grad_(True), ctx.double().requires_grad_(True)
    ref = R.transformer_block(sd, "t", xr, cr, 2, *_tb_mults(blk, 31, 1))
    ref.backward(dy.double())
    with torch.no_grad():
        wrong = R.transformer_block(sd, "t", xr, cr, 2, *_tb_mults(blk, 31, 2))
    blk = blk.cuda()
    ops.dropout_seed(31, 0)
    out, dx, dctx, grads = _tb_run(blk, x, ctx, dy)
    assert ops.dropout_state() == (31, 1)
    _against_float64(f"BasicTransformerBlock {form}", out, ref, wrong, [dx, dctx], [xr.grad, cr.grad], grads, {k[2:]: v.grad for k, v in sd.items()})


def test_transformer_block_checkpoint_is_bit_identical():
    from neurosis_amd import ops

    blk = _tblock().cuda()
    x, ctx, dy = _tb_inputs()
    res = []
    for ck in (False, True):
        blk.checkpoint = ck
        ops.dropout_seed(31, 0)
        xg, cg = x.cuda().requires_grad_(True), ctx.cuda().requires_grad_(True)
        out = blk(xg, cg)
        ops.dropout_draw()
        out.backward(dy.cuda())
        torch.cuda.synchronize()
        res.append((out.detach().clone(), xg.grad.clone(), cg.grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}))
    (o0, dx0, dc0, g0), (o1, dx1, dc1, g1) = res
    assert _same_bits(o0, o1) and torch.equal(dx0, dx1) and torch.equal(dc0, dc1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ------------------------------------------------------------------------------------------------
# 5. the VAE's ResnetBlock
# ------------------------------------------------------------------------------------------------
def _vae_block(p=P):
    from neurosis_amd.modules.diffusion.model import ResnetBlock

    return _randomize(ResnetBlock(in_channels=64, out_channels=128, temb_channels=0, dropout=p), 7)


def _vae_run(blk, x, dy, draw: bool):
    """x, dy NCHW fp32 (bf16 values) -> (y, dx) NCHW, parameter gradients; through fwdb, the training path"""
    from neurosis_amd import ops
    from neurosis_amd.ops import Img

    N, _, H, W = x.shape
    if draw:
        ops.dropout_draw()                                         # (the Encoder / Decoder training forward does this; the block has no forward of its own)
    y, bwd = blk.fwdb(Img(ops.nchw_to_tokens(x.cuda(), 64), N, H, W))
    dx = bwd(ops.nchw_to_tokens(dy.cuda(), 128))
    ops.join_wgrad_stream()
    torch.cuda.synchronize()
    return (ops.tokens_to_nchw(y.t, N, 128, H, W), ops.tokens_to_nchw(dx, N, 64, H, W), {k: p.grad.clone() for k, p in blk.named_parameters()})


def test_vae_resnet_block_against_float64():
    from neurosis_amd import ops

    blk = _vae_block()
    sd = _sd64(blk, "v")
    g = torch.Generator().manual_seed(300)
    x, dy = bf16_round(torch.randn(2, 64, 8, 8, generator=g)), bf16_round(torch.randn(2, 128, 8, 8, generator=g))
    xr = x.double().requires_grad_(True)
    mult = lambda step: R.tokens_to_nchw(R.multiplier(128, 128, P, 41, step, 0), 2, 8, 8)
    ref = R.vae_resnet(sd, "v", xr, mult(1))
    ref.backward(dy.double())
    with torch.no_grad():
        wrong = R.vae_resnet(sd, "v", xr, mult(2))
    blk = blk.cuda()
    ops.dropout_seed(41, 0)
    out, dx, grads = _vae_run(blk, x, dy, draw=True)
    _against_float64("VAE ResnetBlock", out, ref, wrong, [dx], [xr.grad], grads, {k[2:]: v.grad for k, v in sd.items()})
    # the frozen first stage's path has no dropout, whatever the rate
    from neurosis_amd.ops import Img

    with torch.no_grad():
        a = blk.fwd(Img(ops.nchw_to_tokens(x.cuda(), 64), 2, 8, 8)).t
        b = _vae_block(0.0).cuda().fwd(Img(ops.nchw_to_tokens(x.cuda(), 64), 2, 8, 8)).t
    assert _same_bits(a, b) and ops.dropout_state() == (41, 1)


# ------------------------------------------------------------------------------------------------
# 6. neutrality: eval with a rate, and training at rate 0, are today's path
# ------------------------------------------------------------------------------------------------
def _logged(fn):
    from neurosis_amd import lib

    lib.launch_log(1)
    try:
        res = fn()
        names = lib.launched()
    finally:
        lib.launch_log(0)
    return res, names


def _site_runs(kind):
    """(make(p), run(module) -> (tensors, launch names)) for each dropout site"""
    if kind == "resblock":
        x, emb, dy = _rb_inputs()
        return _resblock, lambda m: _logged(lambda: _rb_run(m, x, emb, dy))
    if kind == "transformer":
        x, ctx, dy = _tb_inputs()
        return (lambda p: _tblock(p, checkpoint=False)), lambda m: _logged(lambda: _tb_run(m, x, ctx, dy))
    g = torch.Generator().manual_seed(300)
    x, dy = bf16_round(torch.randn(2, 64, 8, 8, generator=g)), bf16_round(torch.randn(2, 128, 8, 8, generator=g))
    return _vae_block, lambda m: _logged(lambda: _vae_run(m, x, dy, draw=False))


@pytest.mark.parametrize("kind", ["resblock", "transformer", "vae_resnet"])
def test_eval_mode_and_rate_zero_are_the_path_without_dropout(kind, monkeypatch):
    from neurosis_amd import ops

    make, run = _site_runs(kind)
    ops.dropout_seed(5, 9)

    def boom(*a, **k):
        raise AssertionError("a dropout entry point was called on a path without dropout")

    for name in ("dropout_draw", "dropout_fwd", "dropout_mask_like"):
        monkeypatch.setattr(ops, name, boom)
    base, base_names = run(make(0.0).cuda().train())                # training at rate 0
    with_rate = make(P).cuda().eval()                                # a rate, but eval mode (same weights: same seed)
    got, got_names = run(with_rate)
    assert base_names == got_names and len(base_names) > 5 and not [n for n in base_names if "dropout" in n]

    def flat(res):
        return [t for r in res for t in (r.values() if isinstance(r, dict) else [r])]

    for a, b in zip(flat(base), flat(got)):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b)
    monkeypatch.undo()
    assert ops.dropout_state() == (5, 9)                             # nothing drew


# ------------------------------------------------------------------------------------------------
# 7. hipGraph replay: the mask changes on every replay and equals the eager chain's
# ------------------------------------------------------------------------------------------------
UNET_CFG = dict(in_channels=4, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[2], channel_mult=[1, 2], num_head_channels=16,
                use_linear_in_transformer=True, transformer_depth=1, context_dim=32, use_checkpoint=False)           # tests/test_abi.py's tiny UNet


def _graph_steps(graph: bool, n=5):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd import ops
    from neurosis_amd.nn import FlatParamStore

    os.environ["NK_GRAPH"] = "1" if graph else "0"
    try:
        torch.manual_seed(0)
        net = _randomize(D.UNetModel(dropout=0.1, **UNET_CFG), 9).cuda()
        store = FlatParamStore(net.parameters())
        store.state.wgrad_stream = torch.cuda.Stream()
        den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization()).cuda()
        lossfn = D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())
        g = torch.Generator().manual_seed(7)
        x, noise = torch.randn(2, 4, 16, 16, generator=g).cuda(), torch.randn(2, 4, 16, 16, generator=g).cuda()
        sigma, ctx = torch.tensor([0.5, 3.0]).cuda(), torch.randn(2, 7, 32, generator=g).cuda()
        ops.dropout_seed(7)
        losses, grads, replays = [], [], []
        for _ in range(n):
            loss = lossfn._forward(D.OpenAIWrapper(net), den, {"crossattn": ctx}, x, {}, sigmas=sigma, noise=noise)
            loss.mean().backward()
            torch.cuda.synchronize()
            losses.append(loss.detach().clone())
            grads.append(store.grad.clone())
            replays.append(net._nk_graphs.replays if net._nk_graphs is not None else 0)
        return losses, grads, replays, ops.dropout_state()
    finally:
        os.environ.pop("NK_GRAPH", None)


def test_graph_replay_draws_a_new_mask_every_step_and_equals_the_eager_chain():
    loss_g, grad_g, replays, state_g = _graph_steps(True)
    assert state_g == (7, 5)                                         # five micro-batches, five draws -- replayed or not
    assert replays[0] == 0 and replays[1] > 0 and replays[2] > replays[1] and replays[3] > replays[2] and replays[4] > replays[3]
    for i in range(2, 5):                                            # steps 3-5 are replays of ONE captured launch sequence on identical inputs
        for j in range(i + 1, 5):
            assert not torch.equal(loss_g[i], loss_g[j]) and not torch.equal(grad_g[i], grad_g[j])
    loss_e, grad_e, replays_e, state_e = _graph_steps(False)
    assert state_e == (7, 5) and replays_e == [0] * 5
    for i in range(5):
        d = float((grad_g[i] - grad_e[i]).norm() / grad_e[i].norm())
        print(f"[dropout graphs] step {i + 1}: loss {loss_g[i].tolist()} vs eager {loss_e[i].tolist()}; flat gradient relative distance {d:.3e}")
    for i in range(5):
        assert torch.equal(loss_g[i], loss_e[i]), i
        assert torch.equal(grad_g[i], grad_e[i]), i


# ------------------------------------------------------------------------------------------------
# 8. the engine: one draw per micro-batch
# ------------------------------------------------------------------------------------------------
def test_engine_training_step_draws_once_per_micro_batch():
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd import ops
    from neurosis_amd.models import AutoencoderKL, DiffusionEngine
    from tests.golden.fixture_io import load_fixture
    from tests.golden.make_golden import UNET_TINY, VAE_TINY, synth_state_dict

    keys = json.loads((G / "engine_tiny_keys.json").read_text())
    e = load_fixture("engine_tiny")
    net = D.UNetModel(**{**UNET_TINY, "dropout": 0.1})
    net.load_state_dict(synth_state_dict(keys["unet"]))
    vae = AutoencoderKL(embed_dim=4, ddconfig={k: v for k, v in VAE_TINY.items() if k != "embed_dim"})
    vae.load_state_dict({k: v for k, v in synth_state_dict(keys["vae"]).items() if not k.startswith(("encoder.quant_conv", "decoder.post_quant_conv"))})
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization())
    eng = DiffusionEngine(model=net, denoiser=den, first_stage_model=vae, scale_factor=0.13025, input_key="image", vae_batch_size=2,
                          loss_fn=D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())).cuda()
    eng.setup_flat_params()
    batch = lambda: {"image": e["image"].cuda(), "crossattn": e["crossattn"].cuda(), "vector": e["vector"].cuda()}
    ops.dropout_seed(3, 10)
    losses = []
    for i in range(2):
        eng.accumulate(i, last=(i == 1))
        loss = eng.training_step(batch(), i, sigmas=e["sigma"].cuda(), noise=e["noise"].cuda())
        loss.backward()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    g_sum = eng.store.grad.clone()
    eng.optimizer_step(lr=1e-6)
    eng.join_optimizer()
    assert ops.dropout_state() == (3, 12)                            # two micro-batches: two draws (the frozen VAE and the backward draw nothing)
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[0] != losses[1]      # finite; same batch, another mask
    assert bool(torch.isfinite(g_sum).all()) and float(g_sum.norm()) > 0
