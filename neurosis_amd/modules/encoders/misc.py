"""Embedders without a network (`neurosis.modules.encoders.misc`)."""
from __future__ import annotations

from torch import Tensor

from .embedding import AbstractEmbModel


class IdentityEncoder(AbstractEmbModel):
    """Hands its batch entry on unchanged (misc.py:6-11).  A 4-D entry -- an inpainting model's mask and masked-image latents, an
    edit model's source latents -- is filed under "concat" by GeneralConditioner and becomes input channels of the UNet behind the
    latents; `ucg_rate` and `force_zero_embeddings` are the conditioner's business, as for any embedder."""

    def encode(self, x: Tensor) -> Tensor:
        return x

    def forward(self, x: Tensor) -> Tensor:
        return x
