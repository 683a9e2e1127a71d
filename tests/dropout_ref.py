"""The dropout mask of csrc/dropout.hip restated on the CPU: Philox4x32-10 in plain Python and numpy, the keep bits, the bit-exact fp32
arithmetic of nk_dropout, and float64 restatements of the four module sites that take an explicit multiplier tensor (mask / (1 - p)).

The definition (include/neurosis_hip.h, nk_dropout): one Philox call per 8 consecutive logical elements e = row * cols + col; v = e // 8;
counter = (v & 0xffffffff, v >> 32, site, step & 0xffffffff); key = (seed & 0xffffffff, seed >> 32); element j = e % 8 takes the 16-bit half
(word[j >> 1] >> (16 * (j & 1))) & 0xffff and is kept iff half >= thr = round(p * 65536); kept values are multiplied by the fp32 value of
1 / (1 - p)."""
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sdxl_oracle as O

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments
MASK32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Plain-Python Philox4x32 with 10 rounds: ctr four and key two 32-bit words -> four 32-bit words."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def counter_key(v: int, seed: int, step: int, site: int):
    return (v & MASK32, (v >> 32) & MASK32, site & MASK32, step & MASK32), (seed & MASK32, (seed >> 32) & MASK32)


def philox_words(n_vec: int, seed: int, step: int, site: int) -> np.ndarray:
    """[n_vec, 4] uint32: the four output words of vectors v = 0 .. n_vec - 1 (numpy; the same rounds as philox4x32_10)"""
    v = np.arange(n_vec, dtype=np.uint64)
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    c0, c1 = v & m32, v >> s32
    c2 = np.full(n_vec, site & MASK32, dtype=np.uint64)
    c3 = np.full(n_vec, step & MASK32, dtype=np.uint64)
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def consts(p: float):
    """(thr, scale): the integer threshold and the fp32 multiplier the host passes to the kernel"""
    return int(round(p * 65536)), float(np.float32(1.0 / (1.0 - p)))


def halves(n_elems: int, seed: int, step: int, site: int) -> np.ndarray:
    """[n_elems] the 16-bit half of every logical element"""
    words = philox_words((n_elems + 7) // 8, seed, step, site)               # [n_vec, 4]
    h = np.stack([words & np.uint32(0xFFFF), words >> np.uint32(16)], axis=2)   # [n_vec, 4, 2]: element j = 2 * word + half
    return h.reshape(-1)[:n_elems]


def keep_mask(rows: int, cols: int, p: float, seed: int, step: int, site: int) -> torch.Tensor:
    """bool [rows, cols]: True where the element is kept"""
    thr, _ = consts(p)
    return torch.from_numpy(halves(rows * cols, seed, step, site) >= thr).view(rows, cols)


def multiplier(rows: int, cols: int, p: float, seed: int, step: int, site: int) -> torch.Tensor:
    """float64 [rows, cols]: mask * scale, the scale being the fp32 value the kernel multiplies by"""
    return keep_mask(rows, cols, p, seed, step, site).double() * consts(p)[1]


def apply_exact(x: torch.Tensor, keep: torch.Tensor, p: float, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nk_dropout bit for bit on CPU bf16 tensors: kept bf16_rne(fmul_rn(float(x), scale)), dropped +0; with a residual
    bf16_rne(fadd_rn(float(residual), that fp32 product or 0))"""
    scale = torch.tensor(consts(p)[1], dtype=torch.float32)
    m = torch.where(keep, x.float() * scale, torch.zeros((), dtype=torch.float32))
    if residual is not None:
        m = residual.float() + m
    return m.to(torch.bfloat16)


def tokens_to_nchw(mult: torch.Tensor, N: int, H: int, W: int) -> torch.Tensor:
    """a multiplier over the channels-last token matrix [N * H * W, C] as an NCHW tensor"""
    return mult.view(N, H, W, -1).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------
# the four sites in float64 (parameters: a state dict of float64 tensors under prefix p; mult: the multiplier of each site)
# ------------------------------------------------------------------------------------------------
def resblock(sd, p: str, x, emb, mult):
    """ResBlock with out_layers = GroupNorm, SiLU, Dropout, conv (reference openaimodel.py:280-288); mult NCHW like h"""
    h = O.conv(sd, p + ".in_layers.2", F.silu(O.group_norm(sd, p + ".in_layers.0", x, 1e-5)))
    h = h + O.linear(sd, p + ".emb_layers.1", F.silu(emb))[:, :, None, None]
    h = O.conv(sd, p + ".out_layers.3", F.silu(O.group_norm(sd, p + ".out_layers.0", h, 1e-5)) * mult)
    if (p + ".skip_connection.weight") in sd:
        x = O.conv(sd, p + ".skip_connection", x, padding=0)
    return x + h


def transformer_block(sd, p: str, x, context, heads: int, mult_attn1, mult_attn2, mult_ff):
    """BasicTransformerBlock: to_out = [Linear, Dropout] in both attentions, FeedForward = GEGLU, Dropout, Linear (reference
    modules/attention.py:66-71, 207-211).  x [B, L, C]; mult_attn* [B, L, C]; mult_ff [B, L, 4C]"""
    x = x + O.attention(sd, p + ".attn1", O.layer_norm(sd, p + ".norm1", x), None, heads) * mult_attn1
    x = x + O.attention(sd, p + ".attn2", O.layer_norm(sd, p + ".norm2", x), context, heads) * mult_attn2
    a, gate = O.linear(sd, p + ".ff.net.0.proj", O.layer_norm(sd, p + ".norm3", x)).chunk(2, dim=-1)
    return x + O.linear(sd, p + ".ff.net.2", a * F.gelu(gate) * mult_ff)


def vae_resnet(sd, p: str, x, mult):
    """the VAE's ResnetBlock with temb = None: norm2, swish, dropout, conv2 (reference modules/diffusion/model.py:123-126)"""
    h = O.conv(sd, p + ".conv1", F.silu(O.group_norm(sd, p + ".norm1", x, 1e-6)))
    h = O.conv(sd, p + ".conv2", F.silu(O.group_norm(sd, p + ".norm2", h, 1e-6)) * mult)
    if (p + ".nin_shortcut.weight") in sd:
        x = O.conv(sd, p + ".nin_shortcut", x, padding=0)
    return x + h
