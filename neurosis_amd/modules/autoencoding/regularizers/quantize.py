"""`neurosis.modules.autoencoding.regularizers.quantize` on MI355X: the discretization bottleneck of the VQ-VAE / VQGAN first stages.

    VectorQuantizer      codebook trained by gradient:  loss = beta * mean((sg[z_q] - z)^2) + mean((z_q - sg[z])^2)
    EMAVectorQuantizer   codebook as exponential moving averages of the vectors assigned to each code:  loss = beta * mse(sg[z_q], z)

Both keep the reference's constructors, initialisation and state_dict keys.  The hot path is three kernels of csrc/vq.hip: the nearest
code of every latent vector (ops.vq_search: exact fp32 on the matrix pipe, the [N, n_e] distance matrix never exists), the gather
z_q = codebook[idx] with sum((z_q - z)^2) (ops.vq_quantize) and the per-code count and vector sum (ops.vq_code_stats), which feeds the
codebook gradient, the EMA update, the perplexity and the cluster usage.  What is left is codebook- or latent-sized torch arithmetic.

Besides forward(z) -> (z_q, dict) the classes speak the engine's protocol: regularize(z_e, noise=None) -> (z_q, log, bwd) with
bwd(dz, weight) -> dz_e the gradient of <dz, z_q> + weight * log[loss_key] with respect to z_e (z_q is the straight-through
z_e + sg[z_q - z_e]); VectorQuantizer's bwd also writes the codebook gradient into the parameter's gradient slot.

Not built (refused by name): remap= / unknown_index="extra" (index remapping), embedding_weight_norm=True; VectorQuantizerWithInputProjection
does not exist here.  The reference's third class of this file, GumbelQuantizer, lives in .gumbel and resolves as
neurosis_amd.modules.autoencoding.regularizers.GumbelQuantizer, the path the reference's configs name; it is not an attribute of this module.
"""
from __future__ import annotations

from abc import abstractmethod
from typing import Iterator, Optional, Tuple

import torch
from torch import Tensor, nn

from .... import ops
from .base import AbstractRegularizer, perplexity_from_counts


def _refuse_remap(name: str, remap, unknown_index) -> None:
    if remap is not None:
        raise NotImplementedError(f"{name}: remap= (index remapping through a file of used codes) is not built")
    if unknown_index == "extra":
        raise NotImplementedError(f'{name}: unknown_index="extra" belongs to remap=, which is not built')
    if unknown_index != "random" and not isinstance(unknown_index, int):
        raise ValueError(f"{name}: unknown_index is 'random', 'extra' or an integer, got {unknown_index!r}")


class AbstractQuantizer(AbstractRegularizer):
    loss_key: str

    @abstractmethod
    def get_codebook_entry(self, indices: Tensor, shape: Optional[Tuple[int, ...]] = None) -> Tensor:
        raise NotImplementedError(f"{type(self).__name__} does not look codes up")

    def get_trainable_parameters(self) -> Iterator[torch.nn.Parameter]:
        yield from self.parameters()

    @staticmethod
    def _rows(z: Tensor, dim: int) -> Tuple[Tensor, int]:
        """the latent vectors as fp32 rows [N, dim], and H * W of the NCHW route (1 otherwise)"""
        if z.ndim == 4:      # b c h w -> b h w c
            return z.float().permute(0, 2, 3, 1).reshape(-1, dim), z.shape[2] * z.shape[3]
        if z.ndim > 4:
            raise ValueError(f"quantizer input of {z.ndim} dimensions: 4-D (b c h w) or up to 3-D [..., dim] inputs are taken")
        return z.float().reshape(-1, dim), 1


class VectorQuantizer(AbstractQuantizer):
    """The VQ-VAE bottleneck with a codebook trained by gradient: n_e codes of e_dim entries, beta the weight of the commitment term
    (the encoder's pull towards its code)."""

    def __init__(self, n_e: int, e_dim: int, beta: float = 0.25, remap: Optional[str] = None, unknown_index: str = "random",
                 sane_index_shape: bool = False, log_perplexity: bool = False, embedding_weight_norm: bool = False, loss_key: str = "loss/vq"):
        super().__init__()
        if embedding_weight_norm:
            raise NotImplementedError("VectorQuantizer: embedding_weight_norm=True (a weight-normed codebook) is not built")
        _refuse_remap("VectorQuantizer", remap, unknown_index)
        self.n_e, self.e_dim, self.beta, self.loss_key = n_e, e_dim, beta, loss_key
        self.embedding = nn.Embedding(self.n_e, self.e_dim)
        self.embedding.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)
        self.remap, self.used, self.re_embed, self.unknown_index = None, None, n_e, unknown_index
        self.sane_index_shape = sane_index_shape
        self.log_perplexity = log_perplexity

    @torch.no_grad()
    def regularize(self, z_e: Tensor, noise: Optional[Tensor] = None):
        weight = self.embedding.weight
        E = weight.detach()
        rows, hw = self._rows(z_e, self.e_dim)
        rows = rows.contiguous()
        idx = ops.vq_search(rows, E)
        z_q, sumsq = ops.vq_quantize(idx, E, rows, hw)
        z_q = z_q.view(z_e.shape)
        numel = rows.numel()
        mse = sumsq / numel
        log = {}
        stats = []

        def code_stats():
            if not stats:
                stats.append(ops.vq_code_stats(idx, rows, self.n_e))
            return stats[0]

        if self.log_perplexity:
            perplexity, cluster_usage = perplexity_from_counts(code_stats()[0])
            log.update({"perplexity": perplexity, "cluster_usage": cluster_usage})
        log[self.loss_key] = self.beta * mse + mse          # both terms have the same value; they differ in what they differentiate
        ind = idx
        if self.sane_index_shape:
            ind = idx.reshape(z_e.shape[0], z_e.shape[2], z_e.shape[3]) if z_e.ndim == 4 else idx.reshape(z_e.shape[0], -1)
        log["min_encoding_indices"] = ind

        def bwd(dz: Tensor, weight_: float = 0.0) -> Tensor:
            """dz_e = dz + w beta (2 / numel) (z - z_q); codebook gradient w (2 / numel) (count_j e_j - sum_j) into embedding.weight's
            gradient slot in its engine mode (the first micro-batch overwrites -- rows nobody chose come out zero --, later ones add)"""
            w = float(weight_)
            if weight.requires_grad:
                count, total = code_stats()
                dE = (w * 2.0 / numel) * (count.to(torch.float32).unsqueeze(1) * E - total)
                flat = ops.grad_flat(weight).view(self.n_e, self.e_dim)
                flat.add_(dE) if ops.wgrad_mode(weight) == 1 else flat.copy_(dE)
            return dz + (w * self.beta * 2.0 / numel) * (z_e.float() - z_q)

        return z_q, log, bwd

    @torch.no_grad()
    def forward(self, z: Tensor) -> Tuple[Tensor, dict]:
        z_q, log, _ = self.regularize(z)
        return z_q, log

    def get_codebook_entry(self, indices: Tensor, shape: Optional[Tuple[int, ...]] = None) -> Tensor:
        """shape specifying (batch, height, width, channel)"""
        z_q = self.embedding.weight.detach()[indices]
        if shape is not None:
            z_q = z_q.view(shape).permute(0, 3, 1, 2).contiguous()
        return z_q


class EmbeddingEMA(nn.Module):
    """The EMA codebook's state: `weight` [num_tokens, codebook_dim] (normal init), `cluster_size` [num_tokens] (zeros) and `embed_avg` (a copy
    of the weight), all requires_grad=False parameters so that they checkpoint under the reference's keys.  `update` switches the
    training-mode update off."""

    def __init__(self, num_tokens, codebook_dim, decay=0.99, eps=1e-5):
        super().__init__()
        self.decay, self.eps, self.update = decay, eps, True
        init = torch.randn(num_tokens, codebook_dim)
        self.weight = nn.Parameter(init, requires_grad=False)
        self.cluster_size = nn.Parameter(torch.zeros(num_tokens), requires_grad=False)
        self.embed_avg = nn.Parameter(init.clone(), requires_grad=False)

    def forward(self, embed_id):
        return self.weight[embed_id]

    def _average(self, buf: Tensor, new: Tensor) -> None:
        buf.data.mul_(self.decay).add_(new, alpha=1 - self.decay)          # buf <- decay * buf + (1 - decay) * new, in place

    def cluster_size_ema_update(self, new_cluster_size):
        self._average(self.cluster_size, new_cluster_size)

    def embed_avg_ema_update(self, new_embed_avg):
        self._average(self.embed_avg, new_embed_avg)

    def weight_update(self, num_tokens):
        """weight = embed_avg / cluster size, the sizes Laplace-smoothed by eps so that an unused code does not divide by zero"""
        total = self.cluster_size.sum()
        smoothed = (self.cluster_size + self.eps) / (total + num_tokens * self.eps) * total
        self.weight.data.copy_(self.embed_avg / smoothed.unsqueeze(1))


class EMAVectorQuantizer(AbstractQuantizer):
    """The codebook follows the encoder: cluster_size and embed_avg are moving averages of nk_vq_code_stats' count and sum, the weight
    their smoothed quotient; no codebook gradient.  The reference also returns `encodings`, the one-hot [N, n_embed] matrix; here it is
    built only with return_encodings=True (it is the matrix the fused search exists to avoid)."""

    def __init__(self, n_embed: int, embedding_dim: int, beta: float, decay: float = 0.99, eps: float = 1e-5, remap: Optional[str] = None,
                 unknown_index: str = "random", loss_key: str = "loss/vq", return_encodings: bool = False):
        super().__init__()
        _refuse_remap("EMAVectorQuantizer", remap, unknown_index)
        self.codebook_dim, self.num_tokens, self.beta, self.loss_key = embedding_dim, n_embed, beta, loss_key
        self.embedding = EmbeddingEMA(self.num_tokens, self.codebook_dim, decay, eps)
        self.remap, self.used, self.re_embed, self.unknown_index = None, None, n_embed, unknown_index
        self.return_encodings = return_encodings

    def get_trainable_parameters(self) -> Iterator[torch.nn.Parameter]:
        """nothing for an optimizer: the three parameters are requires_grad=False and move by the EMA update in forward"""
        yield from (p for p in self.parameters() if p.requires_grad)

    @torch.no_grad()
    def regularize(self, z_e: Tensor, noise: Optional[Tensor] = None):
        emb = self.embedding
        rows, hw = self._rows(z_e, self.codebook_dim)
        rows = rows.contiguous()
        E = emb.weight.detach()
        idx = ops.vq_search(rows, E)
        z_q, sumsq = ops.vq_quantize(idx, E, rows, hw)       # from the codebook BEFORE this step's update, as the reference
        z_q = z_q.view(z_e.shape)
        count, total = ops.vq_code_stats(idx, rows, self.num_tokens)
        perplexity, _ = perplexity_from_counts(count)
        if self.training and emb.update:
            emb.cluster_size_ema_update(count.to(torch.float32))
            emb.embed_avg_ema_update(total)
            emb.weight_update(self.num_tokens)
        numel = rows.numel()
        log = {self.loss_key: self.beta * (sumsq / numel), "encoding_indices": idx, "perplexity": perplexity}
        if self.return_encodings:
            log["encodings"] = torch.nn.functional.one_hot(idx, self.num_tokens).type(z_e.dtype)

        def bwd(dz: Tensor, weight_: float = 0.0) -> Tensor:
            return dz + (float(weight_) * self.beta * 2.0 / numel) * (z_e.float() - z_q)

        return z_q, log, bwd

    @torch.no_grad()
    def forward(self, z: Tensor) -> Tuple[Tensor, dict]:
        z_q, log, _ = self.regularize(z)
        return z_q, log

    def get_codebook_entry(self, indices: Tensor, shape: Optional[Tuple[int, ...]] = None) -> Tensor:
        z_q = self.embedding.weight.detach()[indices]
        if shape is not None:
            z_q = z_q.view(shape).permute(0, 3, 1, 2).contiguous()
        return z_q
