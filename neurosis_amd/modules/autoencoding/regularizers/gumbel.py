"""`GumbelQuantizer` of `neurosis.modules.autoencoding.regularizers` (reference quantize.py:59-160) on MI355X: the Gumbel-softmax
bottleneck, the one quantizer whose choice of code is stochastic and differentiable.

    GumbelQuantizer      codes drawn by the Gumbel-softmax of projected logits:  loss = kl_weight * KL(softmax(logits) || uniform)

It keeps the reference's constructor, submodules (`proj`, `embed`) and state_dict keys and runs on csrc/gumbel.hip (exact-fp32 logits,
counter-based noise, one row pass forward and one backward) and the bf16 GEMMs.  It speaks the engine's protocol like the quantizers of
.quantize: regularize(z_e, noise=None) -> (z_q, log, bwd), bwd(dz, weight) -> dz_e, the gradients of its three parameters written into
their slots.  It resolves as neurosis_amd.modules.autoencoding.regularizers.GumbelQuantizer, the path the reference's configs name.

Not built (refused by name): remap= / unknown_index="extra" (index remapping); widths that are not multiples of 8."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from .... import ops
from .quantize import AbstractQuantizer, _refuse_remap


class GumbelQuantizer(AbstractQuantizer):
    """The Gumbel-softmax bottleneck (Jang et al. 2016, arXiv:1611.01144): logits = proj(z) over n_embed codes, a soft one-hot
    y = softmax((logits + g) / temperature) with Gumbel noise g, z_q = one_hot(argmax y) @ embed (straight_through, and always in eval) or
    y @ embed, and loss = kl_weight * mean_rows sum_j q_j log(q_j n_embed + 1e-10), q = softmax(logits).  `temperature` is a plain
    attribute: a training loop anneals it between steps.  The noise is injected (regularize(z, noise): fp32 Gumbel values [N, n_embed] or
    [B, n_embed, H, W]) or comes from the counter-based generator under the dropout token open on this thread (one is drawn if none is)."""

    def __init__(self, num_hiddens: int, embedding_dim: int, n_embed: int, straight_through: bool = True, kl_weight: float = 5e-4,
                 temp_init: float = 1.0, remap: Optional[str] = None, unknown_index: str = "random", loss_key: str = "loss/vq"):
        super().__init__()
        _refuse_remap("GumbelQuantizer", remap, unknown_index)
        for name, v, top in (("num_hiddens", num_hiddens, ops.VQ_MAX_D), ("embedding_dim", embedding_dim, None), ("n_embed", n_embed, ops.VQ_MAX_CODES)):
            if v < 8 or v % 8 or (top is not None and v > top):
                raise NotImplementedError(f"GumbelQuantizer: {name} = {v} is not taken: it must be {ops.GUMBEL_WIDTH_RULE}"
                                          + (f" and at most {top}" if top is not None else ""))
        self.loss_key, self.num_hiddens, self.embedding_dim, self.n_embed = loss_key, num_hiddens, embedding_dim, n_embed
        self.straight_through, self.temperature, self.kl_weight = straight_through, temp_init, kl_weight
        self.proj = nn.Conv2d(num_hiddens, n_embed, 1)
        self.embed = nn.Embedding(n_embed, embedding_dim)
        self.remap, self.used, self.re_embed, self.unknown_index = None, None, n_embed, unknown_index

    def _noise_rows(self, noise: Tensor, N: int) -> Tensor:
        if noise.ndim == 4:      # b n h w -> (b h w) n
            noise = noise.permute(0, 2, 3, 1)
        noise = noise.reshape(-1, self.n_embed)
        if noise.shape[0] != N:
            raise ValueError(f"GumbelQuantizer: noise of {noise.shape[0]} rows for {N} latent vectors")
        return noise.float().contiguous()

    @torch.no_grad()
    def regularize(self, z_e: Tensor, noise: Optional[Tensor] = None, temp: Optional[float] = None, return_logits: bool = False):
        n, h, d = self.n_embed, self.num_hiddens, self.embedding_dim
        pw, pb, ew = self.proj.weight, self.proj.bias, self.embed.weight
        if not z_e.is_cuda:
            raise NotImplementedError("GumbelQuantizer: z is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
        hard = self.straight_through if self.training else True          # eval must quantize; the noise is added there too, as the reference
        tau = float(self.temperature if temp is None else temp)
        rows, hw = self._rows(z_e, h)
        rows = rows.contiguous()
        N = rows.shape[0]
        route = {}
        if noise is not None:
            route["noise"] = self._noise_rows(noise, N)
        else:
            tok = ops.dropout_token(required=False)
            if tok is None:
                with ops.dropout_token_scope(None):          # a draw of our own: it does not stay open behind this call
                    tok = ops.dropout_draw(rows.device)
            route.update(token=tok, site=ops.dropout_site(self))
        W, E = ops._phys_flat(pw).view(n, h), ew.detach()
        z_rows, idx, kl, logits, y, b_core = ops.gumbel_quantize(rows, W, pb.detach(), E, ops.w2d(pw), ops.w2d(ew), tau, hard, **route)

        def nchw(t: Tensor, c: int) -> Tensor:
            return t.view(z_e.shape[0], z_e.shape[2], z_e.shape[3], c).permute(0, 3, 1, 2).contiguous() if z_e.ndim == 4 else t.view(*z_e.shape[:-1], c)

        z_q = nchw(z_rows, d)
        log = {self.loss_key: self.kl_weight * kl,
               "indices": idx.view(z_e.shape[0], z_e.shape[2], z_e.shape[3]) if z_e.ndim == 4 else idx.view(z_e.shape[:-1])}
        if return_logits:
            log["logits"] = nchw(logits, n)

        def bwd(dz: Tensor, weight_: float = 0.0) -> Tensor:
            """dz_e of <dz, z_q> + w * log[loss_key]; the gradients of proj.weight, proj.bias and embed.weight go into their slots in the
            engine mode (the first micro-batch overwrites, later ones add)"""
            dz_rows = self._rows(dz, d)[0].contiguous()
            d_rows, dl, dzb = b_core(dz_rows, float(weight_) * self.kl_weight)
            if pw.requires_grad:
                ops.gemm_tn_f32(dl, ops.cast_bf16(rows), ops.grad_flat(pw).view(n, h), ops.wgrad_mode(pw),
                                dbias=ops.grad_flat(pb) if pb.requires_grad else None)
            if ew.requires_grad:
                flat = ops.grad_flat(ew).view(n, d)
                if hard:          # S = one_hot(idx) up to one rounding: dE_j = the sum of the rows of dz that chose code j, in row order
                    dE = ops.vq_code_stats(idx, dz_rows, n)[1]
                    flat.add_(dE) if ops.wgrad_mode(ew) == 1 else flat.copy_(dE)
                else:
                    ops.gemm_tn_f32(y, dzb, flat, ops.wgrad_mode(ew))
            return nchw(d_rows.float(), h)

        return z_q, log, bwd

    @torch.no_grad()
    def forward(self, z: Tensor, temp: Optional[float] = None, return_logits: bool = False) -> Tuple[Tensor, dict]:
        z_q, log, _ = self.regularize(z, None, temp, return_logits)
        return z_q, log

    def get_codebook_entry(self, indices: Tensor, shape: Optional[Tuple[int, ...]] = None) -> Tensor:
        """shape specifying (batch, height, width, channel)"""
        z_q = self.embed.weight.detach()[indices.reshape(-1)]
        if shape is not None:
            z_q = z_q.view(shape).permute(0, 3, 1, 2).contiguous()
        return z_q
