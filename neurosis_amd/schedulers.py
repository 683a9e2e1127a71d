"""Learning-rate schedulers the example configs name under the `neurosis.schedulers` prefix (the prefix swap maps them here).

`LegacyCosineAnnealingWarmupRestarts` restates reference schedulers/cosine.py:114-217 (configs/sdxl/sdxl-te.example.yaml): per parameter
group a linear warm-up from `min_lr` (0 where the group's `initial_lr` is not above it) to `initial_lr * gamma ** cycle`, then a cosine
decay back to `min_lr` over the rest of the cycle; cycles restart, each `cycle_mult` times as long (warm-up excluded).  Host arithmetic on
the optimizer's `param_groups` only.  Two differences: torch 2.10's LRScheduler takes no `verbose` (the argument is accepted and ignored),
and `step(epoch)` past the first cycle with cycle_mult != 1 computes the cycle with math.log(x, cycle_mult) (the reference passes the base
to numpy's log as its `out` argument, which raises).
"""
from __future__ import annotations

import math
from typing import Optional

from torch.optim import Optimizer
from torch.optim.lr_scheduler import LRScheduler


class LegacyCosineAnnealingWarmupRestarts(LRScheduler):
    def __init__(self, optimizer: Optimizer, first_cycle_steps: int, cycle_mult: float = 1.0, min_lr: float | list[float] = 1e-6,
                 warm_up_steps: int = 0, gamma: float = 0.9, last_epoch: int = -1, verbose: bool = False):
        if warm_up_steps >= first_cycle_steps:
            raise ValueError(f"LegacyCosineAnnealingWarmupRestarts: the warm-up ({warm_up_steps} steps) must be shorter than the first cycle "
                             f"({first_cycle_steps} steps)")
        # (the reference's attribute names: LRScheduler.state_dict() saves __dict__, so checkpoints stay interchangeable)
        self.first_cycle_steps = first_cycle_steps
        self.cycle_mult = cycle_mult
        self.max_lrs: list[float] = []
        self.active_lrs: list[float] = []
        self.base_lrs: list[float] = []
        self.min_lrs = min_lr
        self.warm_up_steps = warm_up_steps
        self.gamma = gamma
        self.cur_cycle_steps = first_cycle_steps
        self.step_in_cycle = last_epoch
        self.last_epoch = last_epoch
        self.cycle = 0
        self._last_lr = None
        super().__init__(optimizer, last_epoch)
        self.init_lr()

    def init_lr(self) -> None:
        self.max_lrs.clear()
        self.active_lrs.clear()
        self.base_lrs.clear()
        if not isinstance(self.min_lrs, list):
            self.min_lrs = [self.min_lrs] * len(self.optimizer.param_groups)
        for idx, group in enumerate(self.optimizer.param_groups):
            init_lr = group["initial_lr"]
            base_lr = self.min_lrs[idx] if init_lr > self.min_lrs[idx] else 0.0
            self.max_lrs.append(init_lr)
            self.active_lrs.append(init_lr)
            self.base_lrs.append(base_lr)
            group["lr"] = base_lr

    def get_lr(self) -> list[float]:
        if self.step_in_cycle == -1:
            return self.base_lrs
        if self.step_in_cycle < self.warm_up_steps:
            return [(max_lr - base_lr) * self.step_in_cycle / self.warm_up_steps + base_lr for max_lr, base_lr in zip(self.active_lrs, self.base_lrs)]
        t = (self.step_in_cycle - self.warm_up_steps) / (self.cur_cycle_steps - self.warm_up_steps)
        return [base_lr + (max_lr - base_lr) * (1 + math.cos(t * math.pi)) / 2.0 for max_lr, base_lr in zip(self.active_lrs, self.base_lrs)]

    def step(self, epoch: Optional[int] = None) -> None:
        if epoch is None:
            epoch = self.last_epoch + 1
            self.step_in_cycle = self.step_in_cycle + 1
            if self.step_in_cycle >= self.cur_cycle_steps:
                self.cycle += 1
                self.step_in_cycle = self.step_in_cycle - self.cur_cycle_steps
                self.cur_cycle_steps = int((self.cur_cycle_steps - self.warm_up_steps) * self.cycle_mult) + self.warm_up_steps
        elif epoch >= self.first_cycle_steps:
            if self.cycle_mult == 1.0:
                self.step_in_cycle = epoch % self.first_cycle_steps
                self.cycle = epoch // self.first_cycle_steps
            else:
                n = int(math.log(epoch / self.first_cycle_steps * (self.cycle_mult - 1) + 1, self.cycle_mult))
                self.cycle = n
                self.step_in_cycle = epoch - int(self.first_cycle_steps * (self.cycle_mult ** n - 1) / (self.cycle_mult - 1))
                self.cur_cycle_steps = self.first_cycle_steps * self.cycle_mult ** n
        else:
            self.cur_cycle_steps = self.first_cycle_steps
            self.step_in_cycle = epoch
        for i in range(len(self.active_lrs)):
            self.active_lrs[i] = self.max_lrs[i] * (self.gamma ** self.cycle)
        self.last_epoch = float(math.floor(epoch))
        for group, lr in zip(self.optimizer.param_groups, self.get_lr()):
            group["lr"] = lr
        self._last_lr = [group["lr"] for group in self.optimizer.param_groups]
