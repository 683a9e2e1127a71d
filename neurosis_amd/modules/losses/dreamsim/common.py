"""`neurosis.modules.losses.dreamsim.common`: the small helpers of the DreamSim port."""
from __future__ import annotations

from typing import Callable

import torch
from torch import Tensor, nn


def ensure_tuple(val, n: int = 2) -> tuple:
    if isinstance(val, int):
        return (val,) * n
    if len(val) != n:
        raise ValueError(f"Expected a tuple of {n} values, but got {len(val)}: {val}")
    return tuple(val)


class QuickGELU(nn.Module):
    """x * sigmoid(1.702 x).  In a VisionTransformer the class only NAMES the activation (the towers run nk_gelu_fwd in its quick mode);
    the forward is there for stand-alone use."""

    def forward(self, input: Tensor) -> Tensor:
        return input * torch.sigmoid(1.702 * input)


def get_act_layer(name: str) -> Callable[[], nn.Module]:
    if name == "gelu":
        return nn.GELU
    if name == "quick_gelu":
        return QuickGELU
    raise ValueError(f"Activation layer {name} not supported.")
