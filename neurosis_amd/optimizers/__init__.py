"""MI355X mirror of `neurosis.optimizers` (reference `src/neurosis/optimizers/__init__.py`): the optimizer block of the
example configs (`configs/sdxl/sdxl.example.yaml:158-169`, `configs/sd15/sd15.example.yml`) names
`neurosis.optimizers.Adafactor` and `neurosis.optimizers.AdafactorScheduler`; under the `neurosis.` -> `neurosis_amd.` prefix
swap these resolve here.

Every class here is a real `torch.optim.Optimizer` (so LightningCLI's `OptimizerCallable`, `configure_optimizers`, LR schedulers and
checkpointing accept it) under its upstream constructor, whose `step()` is a fused update on the flat fp32 master / gradient buffers of
a `FlatParamStore`; `_base._FusedOptimizer` holds what they share, and says what happens to parameters that have no store yet.

`Adafactor` keeps the reference class's constructor (`optimizers/adafactor.py:100-131`) over `neurosis_amd.optim.FlatAdafactor`, or, when
the group sets `beta1`, over `neurosis_amd.optim.FlatAdafactorMomentum`: the reference's first moment (`exp_avg`, one more fp32 value per
parameter) kept by the same fused update.  Its hyper-parameters are read when the flat optimizer is built, not at every step, and `step`
is kept per parameter.

`CAME` (`neurosis.optimizers.came.CAME`, reference `optimizers/came.py`) is the fused `neurosis_amd.optim.FlatCAME` under the
reference class's constructor: Adafactor's factored second moment plus a first moment and a factored confidence statistic, 4 B of
state per parameter against AdamW's 8 -- the memory-frugal optimizer with momentum that fine-tuning configs move to.  It lives in
`neurosis_amd.optimizers.came`, where the prefix swap of its class path lands, and is re-exported here.

`AdamW8bit` is bitsandbytes' blockwise 8-bit AdamW (`bitsandbytes.optim.AdamW8bit`, the optimizer of the reference's
`configs/sdxl/sdxl-te.example.yaml`) fused as `neurosis_amd.optim.FlatAdamW8bit` under bitsandbytes' constructor: one byte each for m
and v plus two fp32 absmax per 256 elements, 2.03 B of state per parameter against AdamW's 8.  No prefix swap reaches it: a config that
names `bitsandbytes.optim.AdamW8bit` selects it by changing that `class_path` to `neurosis_amd.optimizers.AdamW8bit` (this package
provides no `bitsandbytes` module).  It lives in `neurosis_amd.optimizers.adamw8bit` and is re-exported here.

`AdamW` is the fused flat AdamW (`nk_adamw_flat`) under `torch.optim.AdamW`'s constructor: not named by the reference's
configs, provided because "any subclass of torch.optim.Optimizer" is what its YAML comment invites.
`HybridOptimizer` / `HybridScheduler` (one optimizer per parameter group) are outside the SD/SDXL example configs and are
not built.
"""
from __future__ import annotations

import math
from typing import Optional

from torch.optim import Optimizer
from torch.optim.lr_scheduler import LambdaLR

from ..optim import FlatAdafactor, FlatAdafactorMomentum
from ._base import _FusedOptimizer, _group_store
from .adamw8bit import AdamW8bit
from .came import CAME

__all__ = ["Adafactor", "AdafactorScheduler", "AdamW", "AdamW8bit", "CAME"]


class Adafactor(_FusedOptimizer):
    """`neurosis.optimizers.Adafactor` (reference optimizers/adafactor.py:100-255), fused."""

    _strict_groups = False

    def __init__(self, params, lr: Optional[float] = None, eps: tuple[float, float] = (1e-30, 1e-3), clip_threshold: float = 1.0,
                 decay_rate: float = -0.8, beta1: Optional[float] = None, weight_decay: float = 0.0, scale_parameter: bool = True,
                 relative_step: bool = True, warmup_init: bool = False):
        if lr is not None and relative_step:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if warmup_init and not relative_step:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
        if beta1 is not None and not 0.0 <= beta1 < 1.0:
            raise ValueError(f"beta1 must be None or in [0, 1), got {beta1}")
        defaults = dict(lr=lr, eps=eps, clip_threshold=clip_threshold, decay_rate=decay_rate, beta1=beta1, weight_decay=weight_decay,
                        scale_parameter=scale_parameter, relative_step=relative_step, warmup_init=warmup_init, differentiable=False)
        super().__init__(params, defaults)

    def _make_flat(self, g: dict) -> FlatAdafactor:
        """Built once from the group's hyper-parameters: step() does not read them again (only `grad_scale` reaches the update)."""
        flat = FlatAdafactor if g["beta1"] is None else FlatAdafactorMomentum
        return flat(_group_store(g, "Adafactor"), lr=g["lr"] if not g["relative_step"] else None, eps=tuple(g["eps"]),
                    clip_threshold=g["clip_threshold"], decay_rate=g["decay_rate"], beta1=g["beta1"], weight_decay=g["weight_decay"],
                    scale_parameter=g["scale_parameter"], relative_step=g["relative_step"], warmup_init=g["warmup_init"],
                    boundaries=g.get("chunk_boundaries"))

    @staticmethod
    def _get_lr(param_group: dict, param_state: dict) -> float:
        """adafactor.py:133-147 (what AdafactorScheduler reports), from the group's hyper-parameters and a state holding
        `step` and `RMS`."""
        rel_step_sz = param_group["lr"]
        if param_group["relative_step"]:
            min_step = 1e-6 * param_state["step"] if param_group["warmup_init"] else 1e-2
            rel_step_sz = min(min_step, 1.0 / math.sqrt(param_state["step"]))
        param_scale = 1.0
        if param_group["scale_parameter"]:
            param_scale = max(param_group["eps"][1], float(param_state["RMS"]))
        return param_scale * rel_step_sz


class AdafactorScheduler(LambdaLR):
    """`neurosis.optimizers.AdafactorScheduler` (adafactor.py:258-291): a proxy that reports `initial_lr` before the first
    step and the optimizer's own per-group lr afterwards (here read from the fused kernel's per-tensor lr table)."""

    def __init__(self, optimizer: Optimizer, initial_lr: float = 0.0):
        self.initial_lr = initial_lr

        def lr_lambda(_):
            return self.initial_lr

        for group in optimizer.param_groups:
            group["initial_lr"] = initial_lr
        super().__init__(optimizer, lr_lambda)
        for group in optimizer.param_groups:
            del group["initial_lr"]

    def get_lr(self):
        opt = self.optimizer
        flats = getattr(opt, "_flat", [])
        lrs = [float(f.lr_t[0]) for f in flats if getattr(f, "step_count", 0) > 0]      # (AdamW's groups count no steps of their own)
        if len(lrs) == 0:
            lrs = self.base_lrs  # if called before stepping
        return lrs


class _StoreAdamW:
    """`FlatParamStore.adamw_step` (the moments live in the store itself) behind the interface of the flat optimizers."""

    def __init__(self, store):
        self.store = store

    def step(self, grad_scale: float = 1.0) -> None:
        self.store.adamw_step(self.lr, self.betas, self.eps, self.weight_decay, grad_scale)

    def state_dict(self) -> dict:
        return self.store.optimizer_state_dict()

    def load_state_dict(self, sd: dict) -> None:
        self.store.load_optimizer_state_dict(sd)


class AdamW(_FusedOptimizer):
    """Fused flat AdamW (`FlatParamStore.adamw_step`, one launch over all parameters) under `torch.optim.AdamW`'s arguments."""

    _strict_groups = False

    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _make_flat(self, g: dict) -> _StoreAdamW:
        return _StoreAdamW(_group_store(g, "AdamW"))

    def _push(self, g: dict, f: _StoreAdamW) -> None:
        f.lr, f.betas, f.eps, f.weight_decay = g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]

    def load_state_dict(self, state_dict: dict) -> None:
        self.bind()         # the state lives in the stores: nothing is held back for a later bind()
        super().load_state_dict(state_dict)
