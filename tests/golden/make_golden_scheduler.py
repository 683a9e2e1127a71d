#!/usr/bin/env python
"""Generates tests/golden/lr_legacy_cosine.json: the learning rates the reference's LegacyCosineAnnealingWarmupRestarts
(schedulers/cosine.py:114-217, the scheduler of configs/sdxl/sdxl-te.example.yaml) sets, step by step, for several parameter groups.

    python tests/golden/make_golden_scheduler.py

The reference class cannot be constructed under the installed torch (2.10): its __init__ passes `verbose` positionally to
LRScheduler.__init__, and torch removed that parameter.  So, for the duration of the run and nothing else, LRScheduler.__init__ is
shimmed to accept and drop that one argument; everything the fixture records then comes from the reference's own init_lr, get_lr and
step.  Cases: the sdxl-te settings over the three groups the engine builds (UNet at the config's lr, the two towers at base_lr 1.0)
for three cycles; a cycle_mult of 2 (cycles double; a group whose initial_lr is below min_lr starts from 0); and explicit
step(epoch) calls (cycle_mult 1: the reference's cycle_mult != 1 branch of step(epoch) raises).
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from tests.golden.make_golden import REF_SRC  # noqa: E402

OUT = Path(__file__).resolve().parent / "lr_legacy_cosine.json"

CASES = [
    # (name, group initial_lrs, scheduler kwargs, explicit epochs or None (= steps() without argument), number of steps)
    ("sdxl_te", [3e-5, 1.0, 1.0], dict(first_cycle_steps=50, cycle_mult=1.0, min_lr=3e-7, warm_up_steps=25, gamma=0.9), None, 160),
    ("mult2", [1e-3, 1e-7], dict(first_cycle_steps=12, cycle_mult=2.0, min_lr=1e-6, warm_up_steps=4, gamma=0.5), None, 100),
    ("list_min", [2e-4, 5e-5], dict(first_cycle_steps=10, cycle_mult=1.0, min_lr=[1e-5, 1e-6], warm_up_steps=0, gamma=0.8), None, 35),
    ("epochs", [1e-4], dict(first_cycle_steps=20, cycle_mult=1.0, min_lr=1e-6, warm_up_steps=5, gamma=0.7), [0, 3, 7, 19, 20, 26, 45, 61, 10], None),
]


def groups(initial_lrs):
    params = [torch.nn.Parameter(torch.zeros(1)) for _ in initial_lrs]
    return [{"params": [p], "lr": lr, "initial_lr": lr} for p, lr in zip(params, initial_lrs)]


def run(cls, initial_lrs, kwargs, epochs, steps):
    opt = torch.optim.SGD(groups(initial_lrs), lr=1.0)
    sched = cls(opt, **kwargs)
    lrs = [[g["lr"] for g in opt.param_groups]]
    for e in (epochs if epochs is not None else [None] * steps):
        sched.step() if e is None else sched.step(e)
        lrs.append([float(g["lr"]) for g in opt.param_groups])
    return lrs


def main():
    from torch.optim.lr_scheduler import LRScheduler

    sys.path.insert(0, str(REF_SRC))
    from neurosis.schedulers.cosine import LegacyCosineAnnealingWarmupRestarts as Ref

    original = LRScheduler.__init__

    def without_verbose(self, optimizer, last_epoch=-1, verbose=None):
        original(self, optimizer, last_epoch)

    LRScheduler.__init__ = without_verbose
    try:
        cases = [{"name": n, "initial_lrs": lrs, "kwargs": kw, "epochs": ep, "steps": st, "lrs": run(Ref, lrs, kw, ep, st)} for n, lrs, kw, ep, st in CASES]
    finally:
        LRScheduler.__init__ = original
    OUT.write_text(json.dumps({"cases": cases}, indent=1) + "\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
