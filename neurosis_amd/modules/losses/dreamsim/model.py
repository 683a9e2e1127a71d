"""`neurosis.modules.losses.dreamsim.model`: DreamSim (Fu et al. 2023) as a frozen perceptual distance.

    d(x, y) = 1 - cos(z(x), z(y)),   z = f / |f| - mean(f / |f|),   f = the cls embedding(s) of one ViT-B/16 tower (DreamsimModel) or of
                                                                    three of them side by side (DreamsimEnsemble: dino | clip1 | clip2)

The reference builds these on diffusers' ModelMixin / ConfigMixin and torchvision's transforms; neither is needed here.  The constructor
arguments are the reference's; `from_pretrained` reads a LOCAL directory in the diffusers layout (config.json plus
diffusion_pytorch_model.safetensors) -- there is no hub access.  `Normalize(mean, std)` is folded into the towers' patch gather
(ops.vit_patchify), `do_resize` is ops.resize_bicubic_aa and its adjoint, and the head is one kernel forward, one backward
(ops.dreamsim_head).  `forward(x[2, B, 3, H, W]) -> d[B]` runs under no_grad; `fwdb(x, recons)` also returns the backward w.r.t. the SECOND
image, the same seam as LPIPS.fwdb: both images go through each tower as one batch, only the reconstruction's half keeps a tape, and the
towers pass gradients through without ever launching a weight-gradient kernel.

`vit_config` (keyword-only) is this package's addition: a dict of VisionTransformer arguments (embed_dim, depth, num_heads, img_size,
num_classes) that override ViT-B's, so that tests can build tiny towers.  As in the reference, the towers' native position table is the
224 x 224 one whatever `image_size` says (its `image_size=` lands in vit_base_dreamsim's unused keyword arguments); `image_size` is the
size `do_resize` resamples to.
"""
from __future__ import annotations

import json
import math
from pathlib import Path
from typing import Optional

import torch
from torch import Tensor, nn

from .... import ops
from .common import ensure_tuple
from .vit import VisionTransformer, vit_base_dreamsim

__all__ = ["DreamsimBackbone", "DreamsimEnsemble", "DreamsimModel"]

CONFIG_NAME, WEIGHTS_NAME = "config.json", "diffusion_pytorch_model.safetensors"
DINO_NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
CLIP_NORM = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))


def _affine(mean, std, rescale: bool, clamp: bool):
    """the patch gather's per-channel transform: (v - mean) / std of v = x, or of v = clamp(x / 2 + 0.5, 0, 1) = clamp(x, -1, 1) / 2 + 0.5"""
    if rescale:
        bound = 1.0 if clamp else math.inf
        return ops.vit_affine([0.5 / s for s in std], [(0.5 - m) / s for m, s in zip(mean, std)], -bound, bound)
    return ops.vit_affine([1.0 / s for s in std], [-m / s for m, s in zip(mean, std)])


class DreamsimBackbone(nn.Module):
    """What DreamsimModel and DreamsimEnsemble share: the configuration round trip, the resize, the head and the fwdb seam."""

    _config_keys: tuple = ()
    image_size: tuple
    do_resize: bool

    # -- configuration (the part of diffusers' ConfigMixin / ModelMixin the loss uses) ----------------
    @property
    def config(self) -> dict:
        return {k: getattr(self, "_cfg_" + k) for k in self._config_keys}

    def _register(self, **kwargs) -> None:
        for k, v in kwargs.items():
            setattr(self, "_cfg_" + k, list(v) if isinstance(v, tuple) else v)

    def save_pretrained(self, path) -> None:
        from safetensors.torch import save_file

        path = Path(path)
        path.mkdir(parents=True, exist_ok=True)
        (path / CONFIG_NAME).write_text(json.dumps({"_class_name": type(self).__name__, **self.config}, indent=2))
        save_file({k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}, str(path / WEIGHTS_NAME))

    @classmethod
    def from_pretrained(cls, path, local_files_only: bool = True, revision: Optional[str] = None, *, vit_config: Optional[dict] = None, **unused):
        """Build from a local directory in the diffusers layout.  A hub name cannot be resolved: there is no hub access."""
        from safetensors.torch import load_file

        root = Path(str(path))
        if not (root.is_dir() and (root / CONFIG_NAME).exists()):
            raise FileNotFoundError(f"{str(path)!r} is not a local directory with a {CONFIG_NAME}: there is no hub access here, so a hub name such as "
                                    f"'neggles/dreamsim' cannot be downloaded.  Fetch the repository elsewhere and pass the path of the directory that "
                                    f"holds {CONFIG_NAME} and {WEIGHTS_NAME} (dreamsim_name_or_path of AutoencoderDreamsim)")
        cfg = {k: v for k, v in json.loads((root / CONFIG_NAME).read_text()).items() if not k.startswith("_")}
        unknown = sorted(set(cfg) - set(cls._config_keys))
        if unknown:
            raise ValueError(f"{root / CONFIG_NAME}: keys {unknown} are not arguments of {cls.__name__} (is this the other DreamSim class?)")
        model = cls(**{k: tuple(v) if isinstance(v, list) else v for k, v in cfg.items()}, vit_config=vit_config)
        model.load_state_dict(load_file(str(root / WEIGHTS_NAME)), strict=True)
        return model.requires_grad_(False).eval()

    def train(self, mode: bool = True):
        return super().train(False)                      # frozen

    # -- the distance -----------------------------------------------------------------------------------
    def _towers(self, rescale: bool, clamp: bool):
        """[(tower, affine, norm flag)] in the order their embeddings are laid side by side"""
        raise NotImplementedError

    def _run(self, x: Tensor, recons: Tensor, rescale: bool, keep_tape: bool):
        if x.shape != recons.shape or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"dreamsim: two [B, 3, H, W] image batches of one shape expected, got {tuple(x.shape)} and {tuple(recons.shape)}")
        if not x.is_cuda:
            raise NotImplementedError("dreamsim: the inputs are CPU tensors; the HIP kernels run on the GPU only, there is no CPU path")
        B = x.shape[0]
        both = torch.cat((x.float(), recons.float()), dim=0).contiguous()
        inside = None
        b_resize, size = None, tuple(x.shape[2:])
        if self.do_resize and tuple(both.shape[2:]) != tuple(self.image_size):
            if rescale:      # the reference clamps x / 2 + 0.5 BEFORE it resizes: clamp here, and let the gather's own clamp go
                inside = (both[B:] >= -1.0) & (both[B:] <= 1.0)
                both = both.clamp(-1.0, 1.0)
            both, b_resize = ops.resize_bicubic_aa(both, self.image_size)      # (its own closure is for both halves; the adjoint below is for one)
        towers = self._towers(rescale, clamp=b_resize is None)
        feats, closures = [], []
        for tower, affine, norm in towers:
            f, b = tower.features(both, affine, norm=norm, tape_from=B if keep_tape else None)
            feats.append(f)
            closures.append(b)
        widths = [f.shape[1] for f in feats]
        f = (feats[0] if len(feats) == 1 else torch.cat(feats, dim=1)).reshape(2, B, sum(widths)).contiguous()
        d, b_head = ops.dreamsim_head(f)
        if not keep_tape:
            return d, None

        def bwd(upstream: Tensor) -> Tensor:
            """upstream [B] -> d sum_b upstream_b d_b / d recons, fp32 NCHW; the towers' input gradients are added in their fixed order"""
            df = b_head(upstream)
            dx, at = None, 0
            for b, w in zip(closures, widths):
                dx = b(df[:, at:at + w].contiguous(), out=dx)
                at += w
            closures.clear()
            if b_resize is not None:
                dx = ops.resize_bicubic_aa_bwd(dx, size)
                if inside is not None:
                    dx = dx * inside
            return dx.contiguous()

        return d, bwd

    @torch.no_grad()
    def fwdb(self, x: Tensor, recons: Tensor, rescale: bool = False):
        """x, recons fp32 NCHW [B, 3, H, W] (in [0, 1]; in [-1, 1] with rescale=True, which maps them through clamp(v / 2 + 0.5, 0, 1) first).
        Returns (d [B] fp32, bwd) with bwd(upstream [B]) -> d sum_b upstream_b d_b / d recons (fp32 NCHW).  x gets no gradient."""
        return self._run(x, recons, rescale, keep_tape=True)

    @torch.no_grad()
    def forward(self, x: Tensor) -> Tensor:
        """x [2, B, 3, H, W] -> d [B] (the reference's forward)"""
        if x.dim() != 5 or x.shape[0] != 2:
            raise ValueError(f"dreamsim: expected [2, B, 3, H, W], got {tuple(x.shape)}")
        return self._run(x[0], x[1], False, keep_tape=False)[0]


def _tower(vit_config: Optional[dict], **kwargs) -> VisionTransformer:
    return vit_base_dreamsim(**{**kwargs, **(vit_config or {})})


class DreamsimModel(DreamsimBackbone):
    _config_keys = ("image_size", "patch_size", "layer_norm_eps", "pre_norm", "act_layer", "img_mean", "img_std", "do_resize")

    def __init__(self, image_size: int = 224, patch_size: int = 16, layer_norm_eps: float = 1e-6, pre_norm: bool = False, act_layer: str = "gelu",
                 img_mean: tuple = (0.485, 0.456, 0.406), img_std: tuple = (0.229, 0.224, 0.225), do_resize: bool = False, *,
                 vit_config: Optional[dict] = None) -> None:
        super().__init__()
        self._register(image_size=image_size, patch_size=patch_size, layer_norm_eps=layer_norm_eps, pre_norm=pre_norm, act_layer=act_layer,
                       img_mean=img_mean, img_std=img_std, do_resize=do_resize)
        self.image_size, self.patch_size = ensure_tuple(image_size, 2), ensure_tuple(patch_size, 2)
        self.layer_norm_eps, self.pre_norm, self.do_resize = layer_norm_eps, pre_norm, do_resize
        self.img_mean, self.img_std = tuple(img_mean), tuple(img_std)
        self.extractor = _tower(vit_config, patch_size=patch_size, layer_norm_eps=layer_norm_eps, num_classes=512 if pre_norm else 0,
                                pre_norm=pre_norm, act_layer=act_layer)

    def _towers(self, rescale: bool, clamp: bool):
        return [(self.extractor, _affine(self.img_mean, self.img_std, rescale, clamp), self.pre_norm)]


class DreamsimEnsemble(DreamsimBackbone):
    _config_keys = ("image_size", "patch_size", "layer_norm_eps", "num_classes", "do_resize")

    def __init__(self, image_size: int = 224, patch_size: int = 16, layer_norm_eps=(1e-6, 1e-5, 1e-5), num_classes=(0, 512, 512),
                 do_resize: bool = False, *, vit_config: Optional[dict] = None) -> None:
        super().__init__()
        if isinstance(layer_norm_eps, float):
            layer_norm_eps = (layer_norm_eps,) * 3
        if isinstance(num_classes, int):
            num_classes = (num_classes,) * 3
        vit_config = dict(vit_config or {})
        width = vit_config.pop("num_classes", None)      # in vit_config: the head width of the towers that have a head
        if width is not None:
            num_classes = tuple(int(width) if n else 0 for n in num_classes)
        self._register(image_size=image_size, patch_size=patch_size, layer_norm_eps=layer_norm_eps, num_classes=num_classes, do_resize=do_resize)
        self.image_size, self.patch_size, self.do_resize = ensure_tuple(image_size, 2), ensure_tuple(patch_size, 2), do_resize
        self.dino = _tower(vit_config, patch_size=patch_size, layer_norm_eps=layer_norm_eps[0], num_classes=num_classes[0], pre_norm=False, act_layer="gelu")
        self.clip1 = _tower(vit_config, patch_size=patch_size, layer_norm_eps=layer_norm_eps[1], num_classes=num_classes[1], pre_norm=True,
                            act_layer="quick_gelu")
        self.clip2 = _tower(vit_config, patch_size=patch_size, layer_norm_eps=layer_norm_eps[2], num_classes=num_classes[2], pre_norm=True, act_layer="gelu")

    def _towers(self, rescale: bool, clamp: bool):
        dino, clip = _affine(*DINO_NORM, rescale, clamp), _affine(*CLIP_NORM, rescale, clamp)
        return [(self.dino, dino, False), (self.clip1, clip, True), (self.clip2, clip, True)]
