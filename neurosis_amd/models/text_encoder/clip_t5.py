"""`FrozenCLIPT5Encoder` of `neurosis.models.text_encoder.clip_t5` (:12-38): a CLIP-L text tower and a T5 encoder side by side, returning
[clip_z, t5_z].  Both are rank 3, so GeneralConditioner files both under "crossattn" and joins them along the channel axis -- which needs
clip_max_length == t5_max_length (the defaults: 77 and 77).

The reference's constructor cannot run as written: it passes `device` positionally into FrozenT5Embedder's second parameter, which is
`max_length`, and then `max_length=` again by keyword (a TypeError).  The evident intent is built: the T5 embedder gets t5_version and
t5_max_length and is moved to `device` with the module.  `clip_config` / `t5_config` replace the config lookups as `config` does on the two
embedders; there is never a hub access."""
from __future__ import annotations

import logging
from typing import Optional

from ...modules.encoders.embedding import AbstractEmbModel
from .clip import FrozenCLIPEmbedder
from .t5 import FrozenT5Embedder

logger = logging.getLogger(__name__)


class FrozenCLIPT5Encoder(AbstractEmbModel):
    def __init__(self, clip_version="openai/clip-vit-large-patch14", t5_version="google/t5-v1_1-xl", device="cuda", clip_max_length=77, t5_max_length=77,
                 clip_config: Optional[dict] = None, t5_config: Optional[dict] = None, **kwargs):
        super().__init__(**kwargs)
        if self.is_trainable:
            raise NotImplementedError("FrozenCLIPT5Encoder(is_trainable=True): its two encoders freeze themselves whatever the flag (as in the reference); "
                                      "train a FrozenT5Embedder / FrozenByT5Embedder (is_trainable=True, freeze=False) or a FrozenCLIPEmbedder instead")
        self.clip_encoder = FrozenCLIPEmbedder(clip_version, device, max_length=clip_max_length, config=clip_config)
        self.t5_encoder = FrozenT5Embedder(t5_version, max_length=t5_max_length, config=t5_config)
        count = lambda m: sum(p.numel() for p in m.parameters())      # noqa: E731
        logger.info(f"{type(self.clip_encoder).__name__} has {count(self.clip_encoder) * 1.0e-6:.2f} M parameters, "
                    f"{type(self.t5_encoder).__name__} comes with {count(self.t5_encoder) * 1.0e-6:.2f} M params.")

    def encode(self, text):
        return self(text)

    def forward(self, text):
        """text, or a pair (clip ids [B, 77], t5 ids [B, L]) where the vocabularies are not on this machine"""
        clip_in, t5_in = text if isinstance(text, tuple) else (text, text)
        return [self.clip_encoder.encode(clip_in), self.t5_encoder.encode(t5_in)]
