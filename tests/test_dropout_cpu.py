"""Dropout without a GPU: the Philox / mask restatement (tests/dropout_ref.py) against published vectors and its own statistics, the
constructors that used to refuse or ignore a dropout rate, the C-ABI bindings and the torch.library op."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from tests import dropout_ref as R

N = 65536
TRIPLES = [(1234, 3, 7), (1234, 4, 7), (1234, 3, 8), (42, 0, 0)]        # (seed, step, site)


def _words(s: str):
    return tuple(int(w, 16) for w in s.split())


@pytest.mark.parametrize("ctr, key, out", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),                                                      # Random123 kat_vectors
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),         # Random123 kat_vectors
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
])
def test_philox4x32_10_known_answers(ctr, key, out):
    assert R.philox4x32_10(_words(ctr), _words(key)) == _words(out)


def test_mask_anchors():
    """seed 1234, step 3, site 7: the words of vector 0 (plain Python and numpy agree) and the first 32 keep bits at p = 0.25"""
    want = _words("11d75256 6c8be0ac 3f9870c0 7fe04ab2")
    assert R.philox4x32_10(*R.counter_key(0, 1234, 3, 7)) == want
    assert tuple(int(w) for w in R.philox_words(1, 1234, 3, 7)[0]) == want
    bits = "".join("1" if b else "0" for b in R.keep_mask(1, 32, 0.25, 1234, 3, 7)[0].tolist())
    assert bits == "10111011111100001011101111001111"
    # the numpy rounds are the plain-Python rounds, also where the high counter word and the high key word are in use
    big_seed = (0xDEADBEEF << 32) | 0x12345678
    for v in (1, 77, 8191):
        assert tuple(int(w) for w in R.philox_words(v + 1, big_seed, 5, 9)[v]) == R.philox4x32_10(*R.counter_key(v, big_seed, 5, 9))
    assert R.philox4x32_10(*R.counter_key((3 << 32) | 5, 1, 2, 3)) == R.philox4x32_10((5, 3, 3, 2), (1, 0))


def test_threshold_and_scale():
    assert R.consts(0.25) == (16384, float(np.float32(4.0 / 3.0)))
    assert R.consts(0.5) == (32768, 2.0)
    assert R.consts(0.1)[0] == 6554
    from neurosis_amd import ops

    for p in (0.1, 0.25, 0.5):
        thr, scale = ops.dropout_consts(p)
        assert (thr, float(np.float32(scale))) == R.consts(p)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
@pytest.mark.parametrize("seed, step, site", TRIPLES)
def test_keep_rate(p, seed, step, site):
    """|kept / N - (1 - thr / 65536)| <= 4 sigma of a binomial proportion"""
    kept = int(R.keep_mask(1, N, p, seed, step, site).sum())
    thr, _ = R.consts(p)
    dev = abs(kept / N - (1.0 - thr / 65536.0))
    sigma = math.sqrt(p * (1.0 - p) / N)
    print(f"keep rate p={p} seed={seed} step={step} site={site}: {kept / N:.5f}, {dev / sigma:.2f} sigma")
    assert dev <= 4.0 * sigma


def test_steps_and_sites_are_independent():
    """at p = 0.5 the masks of two steps, and of two sites, agree on half of their bits (within 4 sigma)"""
    base = R.keep_mask(1, N, 0.5, 1234, 3, 7)
    tol = 4.0 * math.sqrt(0.25 / N)
    for other in (R.keep_mask(1, N, 0.5, 1234, 4, 7), R.keep_mask(1, N, 0.5, 1234, 3, 8)):
        eq = float((base == other).double().mean())
        print(f"equal bits: {eq:.4f}")
        assert abs(eq - 0.5) <= tol


def test_exact_arithmetic_restatement():
    """kept: bf16(x * scale) in fp32; dropped: +0 (also for inf / nan / -0 inputs); the residual is added in fp32 before the one rounding"""
    x = torch.tensor([[1.0, -3.0, float("inf"), float("nan"), -0.0, 0.3, 7.0, -1.5]], dtype=torch.bfloat16)
    keep = torch.tensor([[True, False, False, False, False, True, True, False]])
    y = R.apply_exact(x, keep, 0.25)
    s = np.float32(4.0 / 3.0)
    assert y[0, 0] == torch.tensor(float(np.float32(1.0) * s)).bfloat16() and y[0, 6] == torch.tensor(float(np.float32(7.0) * s)).bfloat16()
    assert torch.equal(y[0, 1:5].view(torch.int16), torch.zeros(4, dtype=torch.int16))          # +0 bit patterns
    r = torch.full_like(x, 0.5)
    yr = R.apply_exact(x, keep, 0.25, r)
    assert yr[0, 1] == 0.5 and yr[0, 0] == torch.tensor(0.5 + float(np.float32(1.0) * s)).bfloat16()


def test_constructors_take_a_dropout_rate():
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.modules.attention import BasicTransformerBlock, CrossAttention, FeedForward, SpatialTransformer
    from neurosis_amd.modules.diffusion.model import Decoder, Encoder, ResnetBlock
    from neurosis_amd.modules.diffusion.openaimodel import ResBlock

    rb = ResBlock(64, 128, 0.25, out_channels=96)
    assert rb.dropout == 0.25 and isinstance(rb.out_layers[2], nn.Dropout) and rb.out_layers[2].p == 0.25
    ff = FeedForward(64, glu=True, dropout=0.25)
    assert isinstance(ff.net[1], nn.Dropout) and ff.net[1].p == 0.25
    ca = CrossAttention(64, context_dim=32, heads=2, dim_head=32, dropout=0.25)
    assert ca.to_out[1].p == 0.25
    vb = ResnetBlock(in_channels=64, out_channels=128, temb_channels=0, dropout=0.25)
    assert isinstance(vb.dropout, nn.Dropout) and vb.dropout.p == 0.25
    assert isinstance(ResnetBlock(in_channels=64, temb_channels=0).dropout, nn.Identity)         # as the reference: Identity at rate 0
    blk = BasicTransformerBlock(128, 2, 64, dropout=0.25, context_dim=64)
    assert [m.dropout_p for m in (blk.attn1, blk.attn2, blk.ff)] == [0.25] * 3
    st = SpatialTransformer(64, 2, 32, depth=1, dropout=0.25, context_dim=32, use_linear=True)
    assert st.transformer_blocks[0].ff.dropout_p == 0.25
    cfg = dict(in_channels=4, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[2], channel_mult=[1, 2], num_head_channels=16,
               use_linear_in_transformer=True, transformer_depth=1, context_dim=32, use_checkpoint=False)
    net = D.UNetModel(dropout=0.25, **cfg)
    sites = [m for m in net.modules() if getattr(m, "dropout_p", 0.0) > 0.0]
    # every ResBlock, and both attentions and the FeedForward of every transformer block, got the rate
    assert sum(isinstance(m, ResBlock) for m in sites) == sum(isinstance(m, ResBlock) for m in net.modules()) > 0
    assert sum(isinstance(m, FeedForward) for m in sites) == sum(isinstance(m, BasicTransformerBlock) for m in net.modules()) > 0
    assert sum(isinstance(m, CrossAttention) for m in sites) == 2 * sum(isinstance(m, BasicTransformerBlock) for m in net.modules())
    assert not [m for m in D.UNetModel(**cfg).modules() if getattr(m, "dropout_p", 0.0) > 0.0]
    dd = dict(ch=32, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[], in_channels=3, resolution=16, z_channels=4, dropout=0.25)
    for model in (Encoder(**dd), Decoder(**dd)):
        blocks = [m for m in model.modules() if isinstance(m, ResnetBlock)]
        assert blocks and all(isinstance(b.dropout, nn.Dropout) and b.dropout_p == 0.25 for b in blocks)


@pytest.mark.parametrize("rate", [1.0, -0.1])
def test_rates_outside_the_half_open_unit_interval_are_refused(rate):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.modules.attention import CrossAttention, FeedForward
    from neurosis_amd.modules.diffusion.model import ResnetBlock
    from neurosis_amd.modules.diffusion.openaimodel import ResBlock

    with pytest.raises(ValueError, match="ResBlock"):
        ResBlock(64, 128, rate)
    with pytest.raises(ValueError, match="FeedForward"):
        FeedForward(64, glu=True, dropout=rate)
    with pytest.raises(ValueError, match="CrossAttention"):
        CrossAttention(64, dropout=rate)
    with pytest.raises(ValueError, match="ResnetBlock"):
        ResnetBlock(in_channels=64, temb_channels=0, dropout=rate)
    with pytest.raises(ValueError, match="UNetModel"):
        D.UNetModel(in_channels=4, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[2], channel_mult=[1, 2],
                    num_head_channels=16, dropout=rate)


def test_site_ids_follow_the_module_order():
    """dropout_open numbers the dropout-bearing modules by their index in the top module's modules() -- nothing but the structure -- and does
    nothing at all for a module in eval mode or without a rate (no GPU is touched here: those paths return before the draw)"""
    from neurosis_amd import ops
    from neurosis_amd.modules.attention import BasicTransformerBlock

    blk = BasicTransformerBlock(128, 2, 64, dropout=0.25, context_dim=64).eval()
    assert ops.dropout_open(blk) is False and "_nk_site" not in blk.ff.__dict__
    assert ops.dropout_open(BasicTransformerBlock(128, 2, 64, dropout=0.0, context_dim=64)) is False
    assert ops.dropout_site(blk.ff) == 0          # a module used on its own is index 0 of its own modules()


def test_bindings_and_torch_op():
    from neurosis_amd import lib, ops
    import neurosis_amd.torch_ops as T

    l = lib.load()
    assert hasattr(l, "nk_dropout") and hasattr(l, "nk_dropout_draw")
    assert len(lib.SIGNATURES["nk_dropout"]) == 13 and len(lib.SIGNATURES["nk_dropout_draw"]) == 3
    assert l.nk_abi_version() == 5
    for name in ("dropout_draw", "dropout_fwd", "dropout_mask_like", "dropout_seed", "dropout_state"):
        assert callable(getattr(ops, name))
    assert "dropout" in T.OPS
    assert str(torch.ops.neurosis_hip.dropout.default._schema).startswith("neurosis_hip::dropout(")
    x = torch.empty(6, 40, dtype=torch.bfloat16, device="meta")
    tok = torch.empty(2, dtype=torch.int64, device="meta")
    for res in (None, x):
        y = torch.ops.neurosis_hip.dropout(x, tok, 0.25, 3, res)
        assert y.shape == x.shape and y.dtype == x.dtype and y.device.type == "meta"
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.neurosis_hip.dropout(torch.zeros(8, 8, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int64), 0.25, 0)
