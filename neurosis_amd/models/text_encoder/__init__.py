"""Frozen text encoders of the conditioner on MI355X: names of `neurosis.models.text_encoder` -- the CLIP towers
(frozen or trained with the UNet) and the frozen T5 / ByT5 encoders.  The image embedder is not built."""
from .clip import CLIPTextTower, FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder2, OpenCLIPTextTower
from .clip_t5 import FrozenCLIPT5Encoder
from .t5 import FrozenByT5Embedder, FrozenT5Embedder, T5EncoderTower

__all__ = ["CLIPTextTower", "FrozenByT5Embedder", "FrozenCLIPEmbedder", "FrozenCLIPT5Encoder", "FrozenOpenCLIPEmbedder2", "FrozenT5Embedder",
           "OpenCLIPTextTower", "T5EncoderTower"]
