"""A plain-torch restatement of the DreamSim ensemble and of AutoencoderDreamsim's formula (reference modules/losses/dreamsim/{vit,model}.py and
modules/autoencoding/losses/dreamsim.py:101-140), driven by a state dict with the ensemble's keys (`dino.*`, `clip1.*`, `clip2.*`).  It runs
in the dtype of the weights it is given (float64 for the yardstick), builds an autograd graph, and uses the ops torch.autocast knows
(F.linear, F.layer_norm, F.scaled_dot_product_attention, F.conv2d), so that running it under torch.autocast("cpu", bfloat16) costs what bf16
compute costs the reference.  tests/test_dreamsim_cpu.py holds it to the fixture the reference itself produced."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

DINO_NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
CLIP_NORM = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
# name -> (pre_norm, quick_gelu, layer-norm eps, final norm applied)
TOWERS = {"dino": (False, False, 1e-6, False), "clip1": (True, True, 1e-5, True), "clip2": (True, False, 1e-5, True)}


def pos_table(pos_embed, n_side: int):
    """VisionTransformer.interpolate_pos_encoding for an n_side x n_side patch grid"""
    N = pos_embed.shape[1] - 1
    if n_side * n_side == N:
        return pos_embed
    side = int(math.sqrt(N))
    grid = pos_embed[:, 1:].reshape(1, side, side, -1).permute(0, 3, 1, 2)
    sf = (n_side + 0.1) / math.sqrt(N)
    grid = F.interpolate(grid, scale_factor=(sf, sf), mode="bicubic", align_corners=False)
    assert grid.shape[-1] == n_side and grid.shape[-2] == n_side
    return torch.cat((pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, n_side * n_side, -1)), dim=1)


def tower(sd: dict, name: str, x, heads: int):
    """the cls embedding [N, width] of normalised images x"""
    pre_norm, quick, eps, final = TOWERS[name]
    w = lambda k: sd[f"{name}.{k}"]                                     # noqa: E731
    has = lambda k: f"{name}.{k}" in sd                                 # noqa: E731
    E = w("cls_token").shape[-1]
    p = w("patch_embed.proj.weight").shape[-1]
    t = F.conv2d(x, w("patch_embed.proj.weight"), w("patch_embed.proj.bias") if has("patch_embed.proj.bias") else None, stride=p)
    n_side = t.shape[-1]
    t = t.flatten(2).transpose(1, 2)
    t = torch.cat((w("cls_token").expand(t.shape[0], -1, -1).to(t.dtype), t), dim=1)
    t = t + pos_table(w("pos_embed"), n_side)
    if pre_norm:
        t = F.layer_norm(t, (E,), w("norm_pre.weight"), w("norm_pre.bias"), eps)
    i = 0
    while has(f"blocks.{i}.norm1.weight"):
        b = f"blocks.{i}."
        h = F.layer_norm(t, (E,), w(b + "norm1.weight"), w(b + "norm1.bias"), eps)
        B, L, _ = h.shape
        qkv = F.linear(h, w(b + "attn.qkv.weight"), w(b + "attn.qkv.bias")).reshape(B, L, 3, heads, E // heads).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(B, L, E)
        t = t + F.linear(a, w(b + "attn.proj.weight"), w(b + "attn.proj.bias"))
        h = F.linear(F.layer_norm(t, (E,), w(b + "norm2.weight"), w(b + "norm2.bias"), eps), w(b + "mlp.fc1.weight"), w(b + "mlp.fc1.bias"))
        h = h * torch.sigmoid(1.702 * h) if quick else F.gelu(h)
        t = t + F.linear(h, w(b + "mlp.fc2.weight"), w(b + "mlp.fc2.bias"))
        i += 1
    if final:
        t = F.layer_norm(t, (E,), w("norm.weight"), w("norm.bias"), eps)
    t = t[:, 0]
    if has("head.weight"):
        t = F.linear(t, w("head.weight"), w("head.bias"))
    return t


def _normalize(x, stats):
    mean, std = (torch.tensor(s, dtype=x.dtype).view(1, 3, 1, 1) for s in stats)
    return (x - mean) / std


def ensemble(sd: dict, inputs, recons, heads: int, rescale: bool = True):
    """({tower: embedding [2B, width]}, d [B]) of images in [-1, 1] (rescale) or [0, 1]"""
    x = torch.cat((inputs, recons), dim=0)
    if rescale:
        x = (x / 2 + 0.5).clamp(0.0, 1.0)
    emb = {name: tower(sd, name, _normalize(x, DINO_NORM if name == "dino" else CLIP_NORM), heads) for name in TOWERS}
    z = torch.cat([emb[name] for name in TOWERS], dim=1)
    z = z.div(z.norm(dim=1, keepdim=True))
    z = z.sub(z.mean(dim=1, keepdim=True)).view(2, inputs.shape[0], -1)
    return emb, 1 - F.cosine_similarity(z[0], z[1], dim=1)


def autoencoder_dreamsim(sd: dict, inputs, recons, heads: int, recon_type: str, recon_weight: float, dreamsim_weight: float, rescale: bool = True):
    """(loss, rec [B], p scalar):  loss = mean_b(recon_weight * rec_b + dreamsim_weight * relu(sum_b' d_b'))  on the clamped images"""
    xi, xr = inputs.clamp(-1.0, 1.0), recons.clamp(-1.0, 1.0)
    rec = ((xi - xr) ** 2 if recon_type == "l2" else (xi - xr).abs()).mean(dim=(1, 2, 3)) * recon_weight
    p = ensemble(sd, xi, xr, heads, rescale)[1].sum().relu() * dreamsim_weight
    return (rec.float() + p.float()).mean(), rec, p
