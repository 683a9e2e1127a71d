"""The autoencoder-training loss CLASSES of the reference, with the reference's constructors, so that a config-5 YAML
(`loss: {class_path: neurosis.modules.autoencoding.losses.GeneralLPIPSWithDiscriminator, init_args: {...}}`) prefix-swaps like the
SDXL one does.

    GeneralLPIPSWithDiscriminator   /root/reference/src/neurosis/modules/autoencoding/losses/discriminator_loss.py:22-88
    AutoencoderLPIPSWithDiscr       /root/reference/src/neurosis/modules/autoencoding/losses/vae_lpips_discr.py:140-200
    AutoencoderPerceptual           the same file, :25-137
    AutoencoderDreamsim             the reference's modules/autoencoding/losses/dreamsim.py:16-152

In the reference these modules own the LPIPS network, the PatchGAN discriminator and the output log-variance, and their `forward`
assembles the loss from torch ops under autograd.  Here they OWN THE SAME SUBMODULES UNDER THE SAME NAMES (so `loss.*` checkpoint
keys line up: `loss.discriminator.*` / `loss.discr.*`, `loss.perceptual_loss.*`, `loss.logvar`) and carry the configuration;
the arithmetic is the fused one of `neurosis_amd.models.autoencoder.AutoencodingEngine`, which reads its settings from the loss
object it is handed (`AutoencodingEngine(loss=<one of these>)`): nll with the learnable log-variance, LPIPS broadcast into the
reconstruction term, the adaptive generator weight from two last-layer weight-gradient norms, hinge / vanilla discriminator
losses with explicit logit gradients, alternating optimizers from `disc_start` on.  Calling the object directly raises: there is
no autograd graph through the HIP decoder for a stand-alone loss call to differentiate.

The resize options (`resize_input` / `resize_target`, `scale_input_to_tgt_size`) cover an autoencoder whose decoder output has another
size than its input: the engine resamples the input to the reconstruction's size, or the reconstruction to the input's, with the antialiased
bicubic resize of `ops.resize_bicubic_aa` (the reference's F.interpolate(mode="bicubic", antialias=True)) and, for the reconstruction, its
explicit adjoint.

Options outside the SD / SDXL autoencoder recipes are refused loudly at construction (3-D inputs, R1 penalty, non-LPIPS perceptual
types) rather than accepted and ignored.
"""
from __future__ import annotations

import logging
from sys import maxsize
from typing import Any, Iterator, Optional, Union

import torch
from torch import nn

from ...losses import LPIPS, NLayerDiscriminator, get_discr_loss_fn, weights_init
from ...losses.dreamsim import DreamsimBackbone, DreamsimEnsemble, DreamsimModel

__all__ = ["AutoencoderDreamsim", "AutoencoderLPIPSWithDiscr", "AutoencoderPerceptual", "GeneralLPIPSWithDiscriminator"]

logger = logging.getLogger(__name__)


def _resize_mode(resize_input: bool, resize_target: bool) -> Optional[str]:
    """the engine's `resize`: "input" (the input is resampled to the reconstruction's size), "target" (the reconstruction to the input's)"""
    if resize_input and resize_target:
        raise ValueError("Only one of resize_input and resize_target can be True")
    return "input" if resize_input else "target" if resize_target else None


def _rec_type(kind) -> str:
    name = str(getattr(kind, "value", kind)).lower()
    if name in ("l2", "mse"):
        return "l2"
    if name in ("l1", "mae"):
        return "l1"
    raise ValueError(f"Unknown reconstruction loss type {kind}")


class _FusedLossConfig(nn.Module):
    """What AutoencodingEngine reads from a loss object (`engine_settings`)."""

    rec_loss_type: str
    rec_weight: float
    perceptual_weight: float
    disc_start: int
    disc_factor: float
    discriminator_weight: float
    disc_loss_name: str
    learn_logvar: bool
    resize: Optional[str] = None

    def engine_settings(self) -> dict:
        return dict(resize=self.resize, rec_loss_type=self.rec_loss_type, rec_weight=self.rec_weight, perceptual_loss=self.perceptual_loss,
                    perceptual_weight=self.perceptual_weight, discriminator=self._discriminator_module(), disc_loss=self.disc_loss_name,
                    disc_start=self.disc_start, disc_factor=self.disc_factor, disc_weight=self.discriminator_weight,
                    logvar=self._logvar_parameter(), learn_logvar=self.learn_logvar, regularization_weights=dict(getattr(self, "regularization_weights", {}) or {}))

    def _discriminator_module(self) -> nn.Module:
        raise NotImplementedError

    def _logvar_parameter(self) -> Optional[nn.Parameter]:
        return None

    def forward(self, *args, **kwargs):
        raise RuntimeError(f"{type(self).__name__} configures the fused loss of neurosis_amd.models.autoencoder.AutoencodingEngine "
                           "(pass it as `loss=`); it is not a stand-alone autograd loss on this backend")


class GeneralLPIPSWithDiscriminator(_FusedLossConfig):
    """discriminator_loss.py:22-88 (constructor), :205-320 (what the engine computes)."""

    def __init__(self, disc_start: int, logvar_init: float = 0.0, disc_num_layers: int = 3, disc_in_channels: int = 3, disc_factor: float = 1.0,
                 disc_weight: float = 1.0, perceptual_weight: float = 1.0, disc_loss: str = "hinge", scale_input_to_tgt_size: bool = False, dims: int = 2,
                 learn_logvar: bool = False, rec_loss_type: str = "l2", rec_weight: float = 1.0,
                 regularization_weights: Union[None, dict[str, float]] = None, additional_log_keys: Optional[list[str]] = None,
                 discriminator_config: Optional[dict] = None, lpips_kwargs: Optional[dict] = None):
        super().__init__()
        if dims != 2:
            raise NotImplementedError("dims > 2 (video autoencoders) is outside the SD / SDXL path")
        if disc_loss not in ("hinge", "vanilla"):
            raise ValueError(f"disc_loss must be one of ['hinge', 'vanilla'], got {disc_loss}")
        self.dims, self.scale_input_to_tgt_size = dims, scale_input_to_tgt_size
        # discriminator_loss.py:240-241 resamples the INPUT to the reconstruction's size: the same as resize_input of the classes below
        self.resize = _resize_mode(bool(scale_input_to_tgt_size), False)
        # `lpips_kwargs` is this package's addition: the reference constructs LPIPS() with its packaged weights; here the calibrated lin
        # weights are named explicitly (modules/losses/perceptual.py) or pretrained=False is passed for synthetic runs
        self.perceptual_loss = LPIPS(**(lpips_kwargs or {})).eval() if perceptual_weight > 0 else None
        self.perceptual_weight = float(perceptual_weight)
        self.logvar = nn.Parameter(torch.ones(size=()) * logvar_init, requires_grad=learn_logvar)
        self.learn_logvar = learn_logvar
        disc_kwargs = dict(input_nc=disc_in_channels, n_layers=disc_num_layers, use_actnorm=False)
        if discriminator_config is not None:
            disc_kwargs.update(discriminator_config)
        self.discriminator = NLayerDiscriminator(**disc_kwargs).apply(weights_init)
        self.disc_start = int(disc_start)
        self.disc_loss_name = disc_loss
        self.disc_loss = get_discr_loss_fn(disc_loss)
        self.disc_factor = float(disc_factor)
        self.discriminator_weight = float(disc_weight)
        self.rec_weight = float(rec_weight)
        self.rec_loss_type = _rec_type(rec_loss_type)
        self.regularization_weights = dict(regularization_weights or {})
        self.forward_keys = ["optimizer_idx", "global_step", "last_layer", "split", "regularization_log"]
        self.additional_log_keys = set(additional_log_keys or [])
        self.additional_log_keys.update(set(self.regularization_weights.keys()))

    def get_trainable_parameters(self) -> Iterator[nn.Parameter]:
        return self.discriminator.parameters()

    def get_trainable_autoencoder_parameters(self) -> Any:
        if self.learn_logvar:
            yield self.logvar
        yield from ()

    def _discriminator_module(self) -> nn.Module:
        return self.discriminator

    def _logvar_parameter(self) -> Optional[nn.Parameter]:
        return self.logvar


class AutoencoderLPIPSWithDiscr(_FusedLossConfig):
    """vae_lpips_discr.py:140-200: l1 / l2 reconstruction + LPIPS + PatchGAN with the discriminator under `discr`; no learnable
    log-variance (the nll reduces to the weighted reconstruction sum per sample)."""

    def __init__(self, recon_type="l1", recon_weight: float = 1.0, perceptual_type="lpips", perceptual_weight: float = 1.0, disc_start: int = -1,
                 disc_factor: float = 1.0, disc_weight: float = 1.0, disc_lambda_r1: float = 0.0, disc_loss="hinge", disc_kwargs: Optional[dict] = None,
                 resize_input: bool = False, resize_target: bool = False, extra_log_keys: Optional[list[str]] = None, lpips_kwargs: Optional[dict] = None):
        super().__init__()
        self.recon_type = recon_type
        self.rec_loss_type = _rec_type(recon_type)
        self.recon_weight = self.rec_weight = float(recon_weight)
        if str(getattr(perceptual_type, "value", perceptual_type)).lower() != "lpips":
            raise NotImplementedError(f"Perceptual loss {perceptual_type} not implemented")
        self.resize = _resize_mode(resize_input, resize_target)
        if disc_lambda_r1:
            raise NotImplementedError("the R1 gradient penalty (disc_lambda_r1) needs a double backward through the discriminator: not built")
        self.perceptual_loss = LPIPS(**(lpips_kwargs or {})).eval() if perceptual_weight > 0 else None
        self.perceptual_weight = float(perceptual_weight)
        self.disc_start = disc_start if disc_start > 0 else maxsize      # negative = never start (the reference's INT64_MAX hack)
        self.disc_factor, self.disc_weight, self.disc_lambda_r1 = float(disc_factor), float(disc_weight), float(disc_lambda_r1)
        self.discriminator_weight = self.disc_weight
        disc_config = dict(input_nc=3, n_layers=3, use_actnorm=False)
        if disc_kwargs is not None:
            disc_config.update(disc_kwargs)
        self.discr = NLayerDiscriminator(**disc_config).apply(weights_init)
        self.disc_loss_name = str(getattr(disc_loss, "value", disc_loss)).lower()
        if self.disc_loss_name not in ("hinge", "vanilla"):
            raise ValueError(f"disc_loss must be one of ['hinge', 'vanilla'], got {disc_loss}")
        self.discr_loss = get_discr_loss_fn(self.disc_loss_name)
        self.learn_logvar = False
        self.resize_input_to_target, self.resize_target_to_input = resize_input, resize_target
        self.forward_keys = ["global_step", "optimizer_idx", "split"]
        self.extra_log_keys = set(extra_log_keys or [])

    def get_trainable_parameters(self) -> Iterator[nn.Parameter]:
        yield from self.discr.parameters()

    def _discriminator_module(self) -> nn.Module:
        return self.discr


class AutoencoderPerceptual(_FusedLossConfig):
    """vae_lpips_discr.py:25-137: l1 / l2 reconstruction + LPIPS, no discriminator and no second optimizer.  Passed as `loss=` it makes the
    engine compute, per step,

        loss = mean_b( recon_weight * rec_b + perceptual_weight * relu(LPIPS_b) )

    rec_b the per-sample mean of |x - xrec| (l1) or (x - xrec)^2 (l2), both images clamped to [-1, 1] first (after the resize, if one is
    configured); the gradient is zero where xrec was clamped.  As written the reference's forward returns the sum of a [B] and a [B, 1, 1, 1]
    tensor, a [B, 1, 1, B] tensor that backward() only takes at B = 1; this is the formula its terms spell out, and it coincides with the
    reference at B = 1.  The log carries `{split}/loss/total`, `/rec` and `/p` as device scalars; the three `*_ema` keys cost the reference
    an `.item()` (a host sync) per step and are not produced (`loss_ema_steps` is kept for the config's sake)."""

    def __init__(self, perceptual_type="lpips", perceptual_weight: float = 1.0, lpips_type: str = "alex", recon_type="l1", recon_weight: float = 1.0,
                 resize_input: bool = False, resize_target: bool = False, loss_ema_steps: int = 64, extra_log_keys: list[str] = [],
                 delay_setup: bool = False, compile: bool = False, lpips_kwargs: Optional[dict] = None):
        super().__init__()
        self.recon_type = recon_type
        self.rec_loss_type = _rec_type(recon_type)
        self.recon_weight = self.rec_weight = float(recon_weight)
        self.resize = _resize_mode(resize_input, resize_target)
        self.resize_input_to_target, self.resize_target_to_input = resize_input, resize_target
        self.perceptual_type = str(getattr(perceptual_type, "value", perceptual_type)).lower()
        if self.perceptual_type != "lpips":
            raise NotImplementedError(f"Perceptual loss {perceptual_type} not implemented")
        self._lpips_type = lpips_type
        self._lpips_kwargs = dict(lpips_kwargs or {})
        self.perceptual_loss: Optional[LPIPS] = None
        self.perceptual_weight = float(perceptual_weight)
        self.loss_ema_steps = int(loss_ema_steps)
        self.forward_keys = ["split"]
        self.extra_log_keys = set(extra_log_keys)
        self._compile = compile
        if compile:
            logger.info("AutoencoderPerceptual(compile=True): ignored, the LPIPS trunk runs on this package's HIP kernels, not through TorchInductor")
        # no discriminator: the settings the adversarial classes share are fixed
        self.disc_start, self.disc_factor, self.discriminator_weight, self.disc_loss_name, self.learn_logvar = maxsize, 0.0, 0.0, "hinge", False
        if delay_setup:
            logger.info("Delaying LPIPS model loading until configure_model() call")
        else:
            self.configure_model()

    def configure_model(self) -> None:
        if self.perceptual_loss is None:
            self.perceptual_loss = LPIPS(**{"pnet_type": self._lpips_type, **self._lpips_kwargs}).eval()      # (lpips_kwargs may name the trunk too; it wins)

    def get_trainable_parameters(self) -> Iterator[nn.Parameter]:
        yield from ()

    def _discriminator_module(self) -> Optional[nn.Module]:
        return None

    def engine_settings(self) -> dict:
        return {**super().engine_settings(), "perceptual_only": True}


class AutoencoderDreamsim(_FusedLossConfig):
    """dreamsim.py:16-152: l1 / l2 reconstruction + the DreamSim distance of frozen ViT-B/16 towers (modules/losses/dreamsim), no discriminator
    and no second optimizer.  Passed as `loss=` it makes the engine compute, per step,

        loss = mean_b( recon_weight * rec_b + dreamsim_weight * relu(sum_b' d_b') )

    rec_b the per-sample mean of |x - xrec| (l1) or (x - xrec)^2 (l2), both images clamped to [-1, 1] first (after the resize, if one is
    configured) and, with rescale_input, mapped to [0, 1] for the towers; the gradient is zero where xrec was clamped.  (The reference adds the
    [B] reconstruction term and the scalar DreamSim term and returns the [B] tensor; this is its mean.)  The log carries `{split}/loss/total`,
    `/rec` and `/p` as device scalars.  `dreamsim_name_or_path` names a LOCAL directory in the diffusers layout (config.json plus
    diffusion_pytorch_model.safetensors): there is no hub access, so the reference's default hub name raises at configure_model().

    `vit_config` (keyword-only) is this package's addition: VisionTransformer arguments that override ViT-B's.  With it and no directory at
    `dreamsim_name_or_path` the towers are built at their seeded initialisation instead of loaded (tests, benchmarks)."""

    perceptual_loss = None             # (what the adversarial classes call their LPIPS: the engine reads `dreamsim_loss` from this class)

    def __init__(self, dreamsim_name_or_path="neggles/dreamsim:ensemble_vitb16", dreamsim_weight: float = 1.0, dreamsim_ensemble: bool = True,
                 recon_type="l1", recon_weight: float = 1.0, resize_input: bool = False, resize_target: bool = False, extra_log_keys: list[str] = [],
                 rescale_input: bool = True, delay_setup: bool = False, dreamsim_compile: bool = False, *, vit_config: Optional[dict] = None):
        super().__init__()
        self.recon_type = recon_type
        self.rec_loss_type = _rec_type(recon_type)
        self.recon_weight = self.rec_weight = float(recon_weight)
        self.resize = _resize_mode(resize_input, resize_target)
        self.resize_input_to_target, self.resize_target_to_input = resize_input, resize_target
        self.rescale_input = bool(rescale_input)
        self._dreamsim_cls = DreamsimEnsemble if dreamsim_ensemble else DreamsimModel
        self._dreamsim_name = str(dreamsim_name_or_path)
        self._vit_config = None if vit_config is None else dict(vit_config)
        self.dreamsim_loss: Optional[DreamsimBackbone] = None
        self.dreamsim_weight = self.perceptual_weight = float(dreamsim_weight)
        self.forward_keys = ["split"]
        self.extra_log_keys = set(extra_log_keys)
        self.dreamsim_compile = dreamsim_compile
        if dreamsim_compile:
            logger.info("AutoencoderDreamsim(dreamsim_compile=True): ignored, the DreamSim towers run on this package's HIP kernels, not through TorchInductor")
        # no discriminator: the settings the adversarial classes share are fixed
        self.disc_start, self.disc_factor, self.discriminator_weight, self.disc_loss_name, self.learn_logvar = maxsize, 0.0, 0.0, "hinge", False
        if delay_setup:
            logger.info("Delaying Dreamsim model loading until configure_model() call")
        else:
            self.configure_model()

    def configure_model(self) -> None:
        if self.dreamsim_loss is None:
            import os

            if self._vit_config is not None and not os.path.isdir(self._dreamsim_name):
                self.dreamsim_loss = self._dreamsim_cls(vit_config=self._vit_config)
            else:
                self.dreamsim_loss = self._dreamsim_cls.from_pretrained(self._dreamsim_name, local_files_only=True, vit_config=self._vit_config)
        self.dreamsim_loss = self.dreamsim_loss.requires_grad_(False).eval()

    def get_trainable_parameters(self) -> Iterator[nn.Parameter]:
        yield from ()

    def _discriminator_module(self) -> Optional[nn.Module]:
        return None

    def engine_settings(self) -> dict:
        return {**super().engine_settings(), "perceptual_only": True, "perceptual_kind": "dreamsim"}
