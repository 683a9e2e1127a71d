from .classed import ClassEmbedder
from .embedding import AbstractEmbModel, GeneralConditioner, PrecomputedEmbedder
from .metadata import ConcatTimestepEmbedderND
from .misc import IdentityEncoder

__all__ = ["AbstractEmbModel", "ClassEmbedder", "GeneralConditioner", "PrecomputedEmbedder", "ConcatTimestepEmbedderND", "IdentityEncoder"]
