"""`neurosis.optimizers.came.CAME` (reference optimizers/came.py:13-224) under the `neurosis.` -> `neurosis_amd.` prefix swap.

Same constructor, defaults and validation as the reference class, and a real `torch.optim.Optimizer` (so LightningCLI's
`OptimizerCallable`, `configure_optimizers`, LR schedulers and checkpointing accept it), but its `step()` is the fused
multi-tensor update of `neurosis_amd.optim.FlatCAME` on the flat fp32 master / gradient buffers (`csrc/came.hip`): a few HIP
launches for the whole UNet instead of a Python loop over ~1 700 tensors.  There is no eager fallback.

Deliberate differences: the fp32 masters' bf16 shadows are written round-to-nearest, not stochastically (`copy_stochastic_`);
`ams_bound=True` and `weight_decouple=False` with a weight decay raise `NotImplementedError`.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.optim import Optimizer

from ..optim import FlatCAME, _came_validate

__all__ = ["CAME"]


class CAME(Optimizer):
    """Confidence-guided Adaptive Memory Efficient Optimization, fused (reference optimizers/came.py)."""

    def __init__(self, params, lr: float = 2e-4, betas: tuple[float, float, float] = (0.9, 0.999, 0.9999), weight_decay: float = 0.0,
                 weight_decouple: bool = True, fixed_decay: bool = False, clip_threshold: float = 1.0, ams_bound: bool = False,
                 eps1: float = 1e-30, eps2: float = 1e-16):
        _came_validate(lr, betas, weight_decay, weight_decouple, eps1, eps2, "neurosis_amd.optimizers.came.CAME")
        if ams_bound:
            raise NotImplementedError("neurosis_amd.optimizers.came.CAME: ams_bound=True is not implemented (it needs a full-size "
                                      "exp_avg_sq_hat; off by default in the reference)")
        self.clip_threshold = clip_threshold
        self.eps1 = eps1
        self.eps2 = eps2
        defaults = dict(lr=lr, betas=betas, weight_decay=weight_decay, weight_decouple=weight_decouple, fixed_decay=fixed_decay,
                        ams_bound=ams_bound, eps1=eps1, eps2=eps2)
        super().__init__(params, defaults)
        self._flat: list[FlatCAME] = []
        self._pending_state: Optional[dict] = None

    def __str__(self) -> str:
        return "CAME"

    # -- binding to the flat buffers --------------------------------------------------------------------
    def bind(self) -> list[FlatCAME]:
        """One FlatCAME per parameter group (each group = one flat store).  Idempotent."""
        from . import _group_store

        if not self._flat:
            for g in self.param_groups:
                if g["ams_bound"]:
                    raise NotImplementedError("neurosis_amd.optimizers.came.CAME: ams_bound=True is not implemented")
                self._flat.append(FlatCAME(_group_store(g, "CAME"), lr=g["lr"], betas=tuple(g["betas"]), weight_decay=g["weight_decay"],
                                           weight_decouple=g["weight_decouple"], fixed_decay=g["fixed_decay"],
                                           clip_threshold=self.clip_threshold, eps1=g["eps1"], eps2=g["eps2"]))
            if self._pending_state is not None:
                sd, self._pending_state = self._pending_state, None
                self._load_flat(sd)
        return self._flat

    @property
    def flat(self) -> FlatCAME:
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
            _came_validate(g["lr"], g["betas"], g["weight_decay"], g["weight_decouple"], g["eps1"], g["eps2"], "neurosis_amd.optimizers.came.CAME")
            f.betas, f.weight_decay, f.fixed_decay = tuple(float(b) for b in g["betas"]), float(g["weight_decay"]), bool(g["fixed_decay"])
            f.eps1, f.eps2 = float(g["eps1"]), float(g["eps2"])
            f.step(grad_scale, lr=g["lr"])
            g["step"] = f.step_count
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Nothing to do, on purpose (see neurosis_amd.optimizers.Adafactor.zero_grad): `.grad` tensors are views of the store's
        flat gradient buffer, overwritten by their producers on the first micro-batch of a step."""

    # -- checkpointing: torch's layout, the reference's per-parameter keys and the group's `step` --------------
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
            raise ValueError(f"CAME.load_state_dict: {len(saved_groups)} parameter groups in the checkpoint, {len(self.param_groups)} here")
        for g, saved in zip(self.param_groups, saved_groups):
            if len(saved.get("params", g["params"])) != len(g["params"]):
                raise ValueError("CAME.load_state_dict: a parameter group's size differs from the checkpoint's")
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
            f.load_state_dict({"state": {int(i) - base: st for i, st in sd.get("state", {}).items() if base <= int(i) < base + n},
                               "param_groups": [{"step": g.get("step", 0)}]})
            base += n
