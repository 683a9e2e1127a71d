"""`neurosis.modules.losses.dreamsim`: the DreamSim perceptual distance on frozen ViT-B/16 towers (model.py, vit.py); the reference's
LoRA-merge utility (utils.py) is not part of this package."""
from .common import QuickGELU, ensure_tuple, get_act_layer
from .model import DreamsimBackbone, DreamsimEnsemble, DreamsimModel
from .vit import VisionTransformer, interpolate_pos_encoding, vit_base_dreamsim

__all__ = ["DreamsimBackbone", "DreamsimEnsemble", "DreamsimModel", "QuickGELU", "VisionTransformer", "ensure_tuple", "get_act_layer",
           "interpolate_pos_encoding", "vit_base_dreamsim"]
