"""`AdamW8bit`: bitsandbytes' blockwise 8-bit AdamW (`bitsandbytes.optim.AdamW8bit`, the optimizer of the reference's
`configs/sdxl/sdxl-te.example.yaml`), fused on the flat buffers.

Same constructor and defaults as `bitsandbytes.optim.AdamW8bit`, and a real `torch.optim.Optimizer` (so LightningCLI's
`OptimizerCallable`, `configure_optimizers`, LR schedulers and checkpointing accept it), but its `step()` is one HIP launch of
`neurosis_amd.optim.FlatAdamW8bit` (`csrc/adamw8bit.hip`) over the whole flat fp32 master / gradient buffer.  The algorithm is
defined in `FlatAdamW8bit`'s docstring; bit-for-bit interchange with bitsandbytes itself is not claimed.  There is no eager fallback.

Not built, and refused loudly: `amsgrad=True`, `block_wise=False` (one absmax per tensor), `percentile_clipping < 100`, `args`
(bitsandbytes' per-module override object) and `is_paged=True` (paged state).  `optim_bits` is accepted and ignored, as in
bitsandbytes' own AdamW8bit, which always keeps 8-bit state.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.optim import Optimizer

from ..optim import FlatAdamW8bit, _adamw_validate

__all__ = ["AdamW8bit"]

_WHO = "neurosis_amd.optimizers.AdamW8bit"


class AdamW8bit(Optimizer):
    """8-bit blockwise AdamW, fused (bitsandbytes.optim.AdamW8bit's constructor)."""

    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, optim_bits: int = 32, args=None, min_8bit_size: int = 4096, percentile_clipping: int = 100,
                 block_wise: bool = True, is_paged: bool = False):
        _adamw_validate(lr, betas, eps, weight_decay)
        if amsgrad:
            raise NotImplementedError(f"{_WHO}: amsgrad=True is not implemented (it needs a third, max-of-v state)")
        if not block_wise:
            raise NotImplementedError(f"{_WHO}: block_wise=False (one absmax per tensor) is not implemented; only the blockwise "
                                      "quantization (256 elements per block) is built")
        if percentile_clipping < 100:
            raise NotImplementedError(f"{_WHO}: percentile_clipping={percentile_clipping} is not implemented (gradient-norm history "
                                      "clipping); only 100 (off) is built")
        if args is not None:
            raise NotImplementedError(f"{_WHO}: `args` (a per-module override object) is not implemented; pass the hyper-parameters directly")
        if is_paged:
            raise NotImplementedError(f"{_WHO}: is_paged=True (paged optimizer state) is not implemented")
        if min_8bit_size < 1:
            raise ValueError(f"Invalid min_8bit_size: {min_8bit_size}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, defaults)
        self.min_8bit_size = int(min_8bit_size)
        self._flat: list[FlatAdamW8bit] = []
        self._pending_state: Optional[dict] = None

    # -- binding to the flat buffers --------------------------------------------------------------------
    def bind(self) -> list[FlatAdamW8bit]:
        """One FlatAdamW8bit per parameter group (each group = one flat store).  Idempotent."""
        from . import _group_store

        if not self._flat:
            for g in self.param_groups:
                self._flat.append(FlatAdamW8bit(_group_store(g, "AdamW8bit"), lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"],
                                                weight_decay=g["weight_decay"], min_8bit_size=self.min_8bit_size))
            if self._pending_state is not None:
                sd, self._pending_state = self._pending_state, None
                self._load_flat(sd)
        return self._flat

    @property
    def flat(self) -> FlatAdamW8bit:
        """The fused optimizer of the first (UNet) group."""
        return self.bind()[0]

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for g, f in zip(self.param_groups, self.bind()):
            # the group's hyper-parameters as they are NOW (an LR scheduler or a loaded checkpoint may have changed them)
            _adamw_validate(g["lr"], g["betas"], g["eps"], g["weight_decay"])
            f.betas, f.eps, f.weight_decay = tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"])
            f.step(grad_scale, lr=g["lr"])
            g["step"] = f.step_count
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Nothing to do, on purpose (see neurosis_amd.optimizers.Adafactor.zero_grad): `.grad` tensors are views of the store's
        flat gradient buffer, overwritten by their producers on the first micro-batch of a step."""

    # -- checkpointing: torch's layout, bitsandbytes' per-parameter keys ------------------------------------------------
    def state_dict(self) -> dict:
        groups, state, base = [], {}, 0
        for gi, g in enumerate(self.param_groups):
            n = len(g["params"])
            packed = {k: v for k, v in g.items() if k != "params"}
            packed["params"] = list(range(base, base + n))
            groups.append(packed)
            if gi < len(self._flat):
                packed["step"] = self._flat[gi].step_count
                for i, st in self._flat[gi].state_dict()["state"].items():
                    state[base + i] = st
            base += n
        if not self._flat and self._pending_state is not None:
            state = self._pending_state["state"]
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict: dict) -> None:
        saved_groups = state_dict.get("param_groups", [])
        if len(saved_groups) != len(self.param_groups):
            raise ValueError(f"AdamW8bit.load_state_dict: {len(saved_groups)} parameter groups in the checkpoint, {len(self.param_groups)} here")
        for g, saved in zip(self.param_groups, saved_groups):
            if len(saved.get("params", g["params"])) != len(g["params"]):
                raise ValueError("AdamW8bit.load_state_dict: a parameter group's size differs from the checkpoint's")
            for k, v in saved.items():
                if k != "params":
                    g[k] = v
        if self._flat:
            self._load_flat(state_dict)
        else:
            self._pending_state = state_dict      # applied when the flat buffers exist (first step / bind())

    def _load_flat(self, sd: dict) -> None:
        base = 0
        for g, f in zip(self.param_groups, self._flat):
            n = len(g["params"])
            f.load_state_dict({"state": {int(i) - base: st for i, st in sd.get("state", {}).items() if base <= int(i) < base + n}})
            base += n
