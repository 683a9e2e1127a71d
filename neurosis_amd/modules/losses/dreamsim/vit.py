"""`neurosis.modules.losses.dreamsim.vit`: the ViT-B/16 towers of DreamSim as FROZEN feature extractors on the HIP kernels.

A tower is a pre-LN transformer over 1 + (H / p)(W / p) tokens.  Its layers are the residual block of the CLIP text towers
(models/text_encoder/clip.py: LayerNorm, packed QKV GEMM, head-dim-64 attention -- non-causal here --, out projection, LayerNorm, fc1,
GELU or quick-GELU, fc2) with ONE difference: the residual stream is fp32.  d = 1 - cos of two nearby embeddings amplifies what a bf16 stream
rounds away at every add, so the GEMMs write their bf16 branch output and ops.vit_add_ln adds it to the fp32 stream and normalises for the
next GEMM in one pass.  What is not a layer is csrc/vit.hip: the patch gather in
front of the patch-embedding GEMM (ops.vit_patchify, which also applies the per-channel input normalisation), the token assembly with the
cls token and the position table (ops.vit_tokens), their adjoints, and the cls row's final LayerNorm and head, which run in fp32
(ops.vit_cls_head).

The state dict is the reference's (timm's): cls_token, pos_embed, patch_embed.proj.*, norm_pre.*, blocks.N.{norm1, attn.qkv, attn.proj,
norm2, mlp.fc1, mlp.fc2}.*, norm.*, head.*.  Parameters are fp32 with one bf16 shadow per matrix (ops.shadow), as for the frozen CLIP and
T5 towers.  There is no training path: `features` runs a batch whose samples from `tape_from` on keep what an INPUT-gradient-only backward
needs -- per layer two dgrad GEMMs per projection pair, nk_layernorm_bwd_dx, nk_gelu_bwd and the attention backward; no weight-gradient
kernel is launched and neither the weight-gradient stream nor a WgradQueue is touched.  Drop rates are accepted and inert (the towers
never leave eval mode).
"""
from __future__ import annotations

import math
from functools import partial
from typing import Callable, Optional

import numpy as np
import torch
from torch import Tensor, nn

from .... import ops
from .common import QuickGELU, ensure_tuple, get_act_layer

__all__ = ["VisionTransformer", "bicubic_axis_matrix", "interpolate_pos_encoding", "vit_base_dreamsim", "vit_weights_init"]

HEAD_DIM = 64       # the attention kernels' forward and backward are taken at head dim 64 (ViT-B: 768 / 12)


def vit_weights_init(module: nn.Module) -> None:
    if isinstance(module, nn.Linear):
        nn.init.trunc_normal_(module.weight, std=0.02)
        if module.bias is not None:
            nn.init.zeros_(module.bias)
    elif isinstance(module, nn.LayerNorm):
        nn.init.ones_(module.weight)
        nn.init.zeros_(module.bias)


# ---------------------------------------------------------------------------------------------------
# the interpolated position table
# ---------------------------------------------------------------------------------------------------
def bicubic_axis_matrix(n_in: int, n_out: int, scale_factor: float) -> np.ndarray:
    """float64 [n_out, n_in]: F.interpolate(mode="bicubic", align_corners=False, antialias=False) along one axis when `scale_factor` is
    PASSED (not derived from the sizes): output i sits at (i + 0.5) / scale_factor - 0.5 and reads the four inputs around it with the
    Keys cubic at a = -0.75, indices clamped to the edge (taps that clamp to one input add up)."""
    a = -0.75

    def inner(x):     # |x| <= 1
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0

    def outer(x):     # 1 < |x| < 2
        return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a

    M = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        src = (i + 0.5) / scale_factor - 0.5
        i0 = math.floor(src)
        t = src - i0
        for k, w in zip((-1, 0, 1, 2), (outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t))):
            M[i, min(max(i0 + k, 0), n_in - 1)] += w
    return M


def interpolate_pos_encoding(pos_embed: Tensor, patch_size: int, height: int, width: int) -> Tensor:
    """The reference's VisionTransformer.interpolate_pos_encoding (DINO's) as a function of the parameter and the image size: fp32
    [1 + n, E] on the host, computed in float64.  The native table comes back unchanged for a square image with the native token count; any
    other square size resamples the sqrt(N) x sqrt(N) grid with scale_factor (n + 0.1) / sqrt(N) per axis; a non-square image raises the
    ValueError the reference's own size check raises for it."""
    table = pos_embed.detach().reshape(pos_embed.shape[-2], pos_embed.shape[-1]).cpu()
    N = table.shape[0] - 1
    h0, w0 = height // patch_size, width // patch_size
    if h0 * w0 == N and height == width:
        return table.float().contiguous()
    side = int(math.sqrt(N))
    if h0 != w0 or side * side != N:
        raise ValueError("Error in positional encoding interpolation.")
    M = bicubic_axis_matrix(side, h0, (h0 + 0.1) / math.sqrt(N))
    if int(side * ((h0 + 0.1) / math.sqrt(N))) != h0:
        raise ValueError("Error in positional encoding interpolation.")
    grid = table[1:].double().numpy().reshape(side, side, -1)
    out = np.einsum("ai,bj,ijd->abd", M, M, grid).reshape(h0 * w0, -1)
    return torch.cat((table[:1].float(), torch.from_numpy(out).float()), dim=0).contiguous()


# ---------------------------------------------------------------------------------------------------
# modules that hold the reference's parameter names
# ---------------------------------------------------------------------------------------------------
class Mlp(nn.Module):
    def __init__(self, in_features: int, hidden_features: int):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(in_features, hidden_features), nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim: int, num_heads: int, qkv_bias: bool):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(nn.Module):
    def __init__(self, dim: int, num_heads: int, mlp_ratio: float, qkv_bias: bool, norm_layer: Callable[[int], nn.Module]):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads, qkv_bias)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans: int, embed_dim: int, bias: bool):
        super().__init__()
        self.img_size, self.patch_size = ensure_tuple(img_size, 2), ensure_tuple(patch_size, 2)
        self.num_patches = (self.img_size[0] // self.patch_size[0]) * (self.img_size[1] // self.patch_size[1])
        self.dynamic_pad = False
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size, bias=bias)


def _linear(x: Tensor, layer: nn.Linear, residual: Optional[Tensor] = None) -> Tensor:
    return ops.gemm_nt(x, ops.w2d(layer.weight), layer.bias, residual=residual)


def _block_forward(x: Tensor, blk: Block, batch: int, quick: bool, tape_from: Optional[int]):
    """The residual block on the fp32 residual stream x [batch * L, E], which it updates IN PLACE (x += attention branch, x += MLP branch);
    the GEMMs and the attention read and write bf16, ops.vit_add_ln sits at each seam.  Returns the tape: the row slices of samples
    tape_from..batch-1 that _block_backward reads (None when tape_from is None)."""
    E = x.shape[1]
    heads = blk.attn.num_heads
    keep = tape_from is not None
    h1, xb, m1, r1 = ops.vit_add_ln(x, None, blk.norm1, copy=keep)
    fused = _linear(h1, blk.attn.qkv)
    attended, _, lse = ops.attention_fwd(fused[:, :E], fused[:, E:2 * E], fused[:, 2 * E:], batch, heads, E // heads, return_lse=True)
    h2, x1b, m2, r2 = ops.vit_add_ln(x, _linear(attended, blk.attn.proj), blk.norm2, copy=keep)
    u = _linear(h2, blk.mlp.fc1)
    ops.vit_add_ln(x, _linear(ops.gelu(u, quick=quick), blk.mlp.fc2), None)
    if not keep:
        return None
    r = tape_from * (x.shape[0] // batch)
    return (xb[r:], m1[r:], r1[r:], fused[r:], attended[r:], lse[tape_from:], x1b[r:], m2[r:], r2[r:], u[r:])


def _block_backward(dx2: Tensor, blk: Block, tape, batch: int, quick: bool) -> Tensor:
    """d x' -> d x through a frozen block: dgrad GEMMs, nk_layernorm_bwd_dx, nk_gelu_bwd and the attention backward -- nothing else"""
    x, m1, r1, fused, attended, lse, x1, m2, r2, u = tape
    E = x.shape[1]
    heads = blk.attn.num_heads
    du = ops.gelu_bwd(ops.gemm_nn(dx2, ops.w2d(blk.mlp.fc2.weight)), u, quick)
    dx1 = ops.layernorm_bwd_dx(ops.gemm_nn(du, ops.w2d(blk.mlp.fc1.weight)), x1, blk.norm2.weight, m2, r2, dx_add=dx2)
    dattended = ops.gemm_nn(dx1, ops.w2d(blk.attn.proj.weight))
    dfused = torch.empty_like(fused)
    ops.attention_bwd(fused[:, :E], fused[:, E:2 * E], fused[:, 2 * E:], attended, lse, dattended, batch, heads, E // heads,
                      dfused[:, :E], dfused[:, E:2 * E], dfused[:, 2 * E:])
    return ops.layernorm_bwd_dx(ops.gemm_nn(dfused, ops.w2d(blk.attn.qkv.weight)), x, blk.norm1.weight, m1, r1, dx_add=dx1)


class VisionTransformer(nn.Module):
    """The reference's VisionTransformer (its constructor arguments, its state dict), frozen.  `norm_layer` must build an nn.LayerNorm and
    `act_layer` be nn.GELU or QuickGELU (get_act_layer): the kernels behind them are fixed."""

    def __init__(self, img_size=224, patch_size=16, in_chans: int = 3, num_classes: int = 0, embed_dim: int = 768, depth: int = 12,
                 num_heads: int = 12, mlp_ratio: float = 4.0, qkv_bias: bool = False, pre_norm: bool = False, drop_rate: float = 0.0,
                 attn_drop_rate: float = 0.0, drop_path_rate: float = 0.0, norm_layer: Callable[[int], nn.Module] = nn.LayerNorm,
                 act_layer: Callable[[], nn.Module] = nn.GELU, skip_init: bool = False, dynamic_pad: bool = False, **kwargs):
        super().__init__()
        if dynamic_pad:
            raise NotImplementedError("dynamic_pad=True is not built: the patch gather (ops.vit_patchify) takes images whose height and width are "
                                      "multiples of the patch size")
        if in_chans != 3:
            raise NotImplementedError(f"in_chans={in_chans}: the patch gather is built for RGB images")
        if embed_dim != num_heads * HEAD_DIM:
            raise NotImplementedError(f"embed_dim / num_heads must be {HEAD_DIM} (the towers' attention runs at head dim {HEAD_DIM}), got {embed_dim} / {num_heads}")
        if act_layer not in (nn.GELU, QuickGELU):
            raise ValueError(f"act_layer must be nn.GELU or QuickGELU (get_act_layer('gelu' | 'quick_gelu')), got {act_layer!r}")
        patch = ensure_tuple(patch_size, 2)
        if patch[0] != patch[1] or patch[0] % 8:
            raise NotImplementedError(f"patch_size must be square and a multiple of 8, got {patch_size}")
        self.img_size, self.patch_size, self.num_classes = img_size, patch_size, num_classes
        self.num_features = self.embed_dim = embed_dim
        self.depth, self.pre_norm, self.quick_gelu = depth, pre_norm, act_layer is QuickGELU
        # accepted and inert: the towers are always in eval mode
        self.drop_rate, self.attn_drop_rate, self.drop_path_rate = drop_rate, attn_drop_rate, drop_path_rate
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim, bias=not pre_norm)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        self.norm_pre = norm_layer(embed_dim) if pre_norm else nn.Identity()
        self.blocks = nn.ModuleList(Block(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer) for _ in range(depth))
        self.norm = norm_layer(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        for m in (self.norm, *([self.norm_pre] if pre_norm else [])):
            if not isinstance(m, nn.LayerNorm):
                raise ValueError(f"norm_layer must build an nn.LayerNorm, got {type(m).__name__}")
        if not skip_init:
            self.reset_parameters()
        self.requires_grad_(False).eval()
        self._pos_cache: dict = {}
        self._patch_w = None

    def reset_parameters(self) -> None:
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.apply(vit_weights_init)

    def train(self, mode: bool = True):
        return super().train(False)                      # frozen: eval mode is the only mode

    def get_intermediate_layers(self, *args, **kwargs):
        raise NotImplementedError("get_intermediate_layers is not built: the DreamSim loss reads the cls embedding only")

    # -- host-side caches ------------------------------------------------------------------------------
    def interpolate_pos_encoding(self, height: int, width: int) -> Tensor:
        """the position table [1 + n, E] for a height x width image, fp32 on the host (module-level interpolate_pos_encoding)"""
        return interpolate_pos_encoding(self.pos_embed, ensure_tuple(self.patch_size, 2)[0], height, width)

    def pos_table(self, height: int, width: int) -> Tensor:
        """interpolate_pos_encoding on the parameters' device, computed once per size (and per value of pos_embed).  The first use copies from
        the host, which a stream capture cannot record."""
        key = (height, width, str(self.pos_embed.device), ops._param_stamp(self.pos_embed))
        hit = self._pos_cache.get(key)
        if hit is None:
            if ops.capturing() or (self.pos_embed.is_cuda and torch.cuda.is_current_stream_capturing()):
                raise RuntimeError(f"the position table for {height} x {width} images is not on {self.pos_embed.device} yet and a stream capture cannot "
                                   "copy it there; run the tower once eagerly at this size (or call pos_table) before capturing")
            self._pos_cache.clear()
            hit = self._pos_cache[key] = self.interpolate_pos_encoding(height, width).to(self.pos_embed.device)
        return hit

    def _patch_weight(self) -> Tensor:
        """patch_embed.proj.weight.view(E, 3 p p) as the bf16 GEMM operand (columns already in the patch gather's (c, ky, kx) order)"""
        w = self.patch_embed.proj.weight
        stamp = ops._param_stamp(w)
        if self._patch_w is None or self._patch_w[0] != stamp:
            self._patch_w = (stamp, ops.cast_bf16(w.detach().reshape(w.shape[0], -1).float().contiguous()))
        return self._patch_w[1]

    # -- the tower ---------------------------------------------------------------------------------------
    def features(self, x: Tensor, affine, norm: bool = True, tape_from: Optional[int] = None):
        """x fp32 NCHW [N, 3, H, W] -> (embedding fp32 [N, num_classes or E], bwd).  `affine` (ops.vit_affine) is the per-channel input
        transform the patch gather applies.  With tape_from = s, bwd(d embedding[s:] fp32, out=None) returns d / d x[s:] (fp32 NCHW, ADDED to
        `out` when given); without, bwd is None and nothing is kept."""
        N, _, H, W = x.shape
        p = ensure_tuple(self.patch_size, 2)[0]
        rows = ops.vit_patchify(x, p, affine)
        L = rows.shape[0] // N + 1
        patches = ops.gemm_nt(rows, self._patch_weight(), self.patch_embed.proj.bias)
        t = ops.vit_tokens(patches, self.cls_token.reshape(-1), self.pos_table(H, W), N)
        s = tape_from
        pre = None
        if self.pre_norm:                  # its output IS the stream: fp32
            t, t_in, m0, r0 = ops.vit_add_ln(t, None, self.norm_pre, copy=s is not None, y_f32=True)
            pre = None if s is None else (t_in[s * L:], m0[s * L:], r0[s * L:])
        tapes = [_block_forward(t, blk, N, self.quick_gelu, s) for blk in self.blocks]      # (t is updated in place)
        # the cls row's final LayerNorm and head run in fp32 on the fp32 parameters (ops.vit_cls_head): 1 - cos amplifies what they round away
        emb, b_head = ops.vit_cls_head(t, N, self.norm if norm else None, self.head if isinstance(self.head, nn.Linear) else None, tape_from=s)
        if s is None:
            return emb, None
        x_taped = x[s:]
        n_taped = N - s
        first_rows = torch.zeros(n_taped, dtype=torch.int64, device=x.device)

        def bwd(dout: Tensor, out: Optional[Tensor] = None) -> Tensor:
            d = b_head(dout)
            d = ops.gather_rows_bwd(d, first_rows, L)                      # the cls rows' gradient into a zero token matrix
            for blk, tape in zip(reversed(self.blocks), reversed(tapes)):
                d = _block_backward(d, blk, tape, n_taped, self.quick_gelu)
            if pre is not None:
                d = ops.layernorm_bwd_dx(d, pre[0], self.norm_pre.weight, pre[1], pre[2])
            drows = ops.gemm_nn(ops.vit_tokens_bwd(d, n_taped), self._patch_weight())
            return ops.vit_patchify_bwd(drows, x_taped, p, affine, out=out)

        return emb, bwd

    @torch.no_grad()
    def forward(self, x: Tensor, norm: bool = True) -> Tensor:
        """the reference's forward(x, norm): the cls embedding (through `norm` when asked, through the head when there is one) of an image batch
        that is ALREADY normalised, fp32 [N, num_classes or E]"""
        return self.features(x.float().contiguous(), ops.vit_affine((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), norm=norm)[0]


def vit_base_dreamsim(patch_size: int = 16, layer_norm_eps: float = 1e-6, num_classes: int = 512, act_layer="gelu", **kwargs) -> VisionTransformer:
    """ViT-B/16 as DreamSim uses it.  embed_dim / depth / num_heads may be overridden through kwargs (this package's addition, for tiny test
    towers); the reference fixes them at 768 / 12 / 12."""
    if isinstance(act_layer, str):
        act_layer = get_act_layer(act_layer)
    shape = dict(embed_dim=768, depth=12, num_heads=12)
    shape.update({k: kwargs.pop(k) for k in list(kwargs) if k in shape})
    return VisionTransformer(patch_size=patch_size, num_classes=num_classes, mlp_ratio=4, qkv_bias=True,
                             norm_layer=partial(nn.LayerNorm, eps=layer_norm_eps), act_layer=act_layer, **shape, **kwargs)
