"""Network wrappers with the reference's names (`neurosis.modules.diffusion.wrappers`, :7-40): the denoiser calls
`wrapper(x, t, cond)`, the wrapper unpacks the conditioning dict into the UNet's keyword arguments."""
from __future__ import annotations

import torch
from torch import Tensor, nn

from .openaimodel import UNetModel


class IdentityWrapper(nn.Module):
    def __init__(self, diffusion_model: UNetModel, compile_model: bool = False, **kwargs):
        super().__init__()
        if compile_model:
            raise NotImplementedError("compile_model: the MI355X path launches HIP kernels / hipGraphs directly; there is no tracing compiler")
        self.diffusion_model = diffusion_model

    def forward(self, *args, **kwargs):
        return self.diffusion_model(*args, **kwargs)


class OpenAIWrapper(IdentityWrapper):
    """cond keys: "concat" (extra input channels), "crossattn" (context tokens), "vector" (pooled / size embedding)."""

    @staticmethod
    def concat_of(cond: dict):
        """the channel-concat conditioning of `cond`, or None when there is none (an empty tensor means none, as in forward)"""
        extra = cond.get("concat")
        return None if extra is None or (torch.is_tensor(extra) and extra.numel() == 0) else extra

    def fused_unet(self, inputs: Tensor, cond: dict, extra_inputs: dict):
        """The bare UNetModel when this call can take the fused HIP path (device latents, no extra network inputs: nk_edm_prepare /
        nk_sample_prepare feed the UNet's first conv directly), else None.  Channel-concat conditioning (inpainting, edit, upscale
        models) stays on the path when it is a 4-D tensor on the latents' device with their B, H, W that needs no gradient: the
        _cat kernels write it behind the latents.  Its channels must fill the UNet's in_channels: anything else is a ValueError here
        instead of a shape error inside the first conv.  A 5-D (video) entry or one that requires grad takes the generic route."""
        unet = self.diffusion_model
        if not isinstance(unet, UNetModel) or not inputs.is_cuda or extra_inputs:
            return None
        extra = self.concat_of(cond)
        if extra is None:
            return unet
        if not torch.is_tensor(extra) or extra.dim() != 4 or inputs.dim() != 4 or extra.requires_grad or extra.device != inputs.device:
            return None
        if extra.shape[0] != inputs.shape[0] or extra.shape[2:] != inputs.shape[2:]:
            return None
        if inputs.shape[1] + extra.shape[1] != unet.in_channels:
            raise ValueError(f"OpenAIWrapper: {inputs.shape[1]} latent + {extra.shape[1]} concat channels = {inputs.shape[1] + extra.shape[1]}, "
                             f"but the UNet has in_channels = {unet.in_channels}")
        return unet

    def forward(self, x: Tensor, t: Tensor, c: dict, **kwargs) -> Tensor:
        # other keys in `c` are ignored, as in the reference
        extra = c.get("concat")
        net_in = x if extra is None or extra.numel() == 0 else torch.cat([x, extra.to(x.dtype)], dim=1)
        return self.diffusion_model(net_in, timesteps=t, context=c.get("crossattn"), y=c.get("vector"), **kwargs)
