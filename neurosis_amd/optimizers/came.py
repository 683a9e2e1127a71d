"""`neurosis.optimizers.came.CAME` (reference optimizers/came.py:13-224) under the `neurosis.` -> `neurosis_amd.` prefix swap: the
reference class's constructor, defaults and validation over the fused multi-tensor update of `neurosis_amd.optim.FlatCAME`
(`csrc/came.hip`).  Binding, stepping and checkpoints are `_FusedOptimizer`'s; `step` is kept in the group, as the reference does.

Deliberate differences: the fp32 masters' bf16 shadows are written round-to-nearest, not stochastically (`copy_stochastic_`);
`ams_bound=True` and `weight_decouple=False` with a weight decay raise `NotImplementedError`.
"""
from __future__ import annotations

from ..optim import FlatCAME, _came_validate
from ._base import _FusedOptimizer, _group_store

__all__ = ["CAME"]

_WHO = "neurosis_amd.optimizers.came.CAME"


class CAME(_FusedOptimizer):
    """Confidence-guided Adaptive Memory Efficient Optimization, fused (reference optimizers/came.py)."""

    def __init__(self, params, lr: float = 2e-4, betas: tuple[float, float, float] = (0.9, 0.999, 0.9999), weight_decay: float = 0.0,
                 weight_decouple: bool = True, fixed_decay: bool = False, clip_threshold: float = 1.0, ams_bound: bool = False,
                 eps1: float = 1e-30, eps2: float = 1e-16):
        _came_validate(lr, betas, weight_decay, weight_decouple, eps1, eps2, _WHO)
        if ams_bound:
            raise NotImplementedError(f"{_WHO}: ams_bound=True is not implemented (it needs a full-size "
                                      "exp_avg_sq_hat; off by default in the reference)")
        self.clip_threshold = clip_threshold
        self.eps1 = eps1
        self.eps2 = eps2
        defaults = dict(lr=lr, betas=betas, weight_decay=weight_decay, weight_decouple=weight_decouple, fixed_decay=fixed_decay,
                        ams_bound=ams_bound, eps1=eps1, eps2=eps2)
        super().__init__(params, defaults)

    def __str__(self) -> str:
        return "CAME"

    def _make_flat(self, g: dict) -> FlatCAME:
        if g["ams_bound"]:
            raise NotImplementedError(f"{_WHO}: ams_bound=True is not implemented")
        return FlatCAME(_group_store(g, "CAME"), lr=g["lr"], betas=tuple(g["betas"]), weight_decay=g["weight_decay"],
                        weight_decouple=g["weight_decouple"], fixed_decay=g["fixed_decay"], clip_threshold=self.clip_threshold,
                        eps1=g["eps1"], eps2=g["eps2"])

    def _push(self, g: dict, f: FlatCAME) -> None:
        _came_validate(g["lr"], g["betas"], g["weight_decay"], g["weight_decouple"], g["eps1"], g["eps2"], _WHO)
        f.lr, f.betas, f.weight_decay = float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["weight_decay"])
        f.fixed_decay, f.eps1, f.eps2 = bool(g["fixed_decay"]), float(g["eps1"]), float(g["eps2"])

    def _group_extras(self, f: FlatCAME) -> dict:
        return {"step": f.step_count}       # the reference keeps the step count in the group, and FlatCAME reads it from there on load
