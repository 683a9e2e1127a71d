#!/usr/bin/env python
"""Generates tests/golden/came_steps.{json,safetensors}: four steps of the REFERENCE's CAME (neurosis.optimizers.came.CAME,
optimizers/came.py) on the mixed parameter set of `make_golden.adafactor_case`, run on the CPU in the authoring container.

    python tests/golden/make_golden_came.py

Inputs (initial values and every step's gradients) are bf16-exact and shared by the three cases; they are stored once, as
bf16, and the tests read them back with `load_came_case`.

The reference's came.py imports `pytorch_optimizer`, which this image lacks.  Before importing it, this script registers a
minimal stand-in for the four names it takes from that package: `NoSparseGradientError`, the type aliases, and a `BaseOptimizer`
whose `validate_*` methods do nothing and whose `apply_weight_decay` restates that package's documented behaviour (decoupled:
p *= 1 - wd * (1 if fixed_decay else lr); otherwise grad += wd * p).  The stand-in is test scaffolding, recorded in the fixture's
JSON; everything that computes the step is the reference's own code.  Case `default` has wd = 0 and uses the stand-in only for
a multiply by one; cases `decay` and `fixed` depend on its weight-decay rule.
"""
from __future__ import annotations

import inspect
import sys
import types
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from tests.golden.fixture_io import save_fixture  # noqa: E402
from tests.golden.make_golden import import_reference  # noqa: E402

SHAPES = [(48, 32), (40, 64), (300, 8), (16, 8, 3, 3), (8, 16, 1, 1), (32,), (7,), (1200,)]
GRAD_MAGNITUDES = [0.1, 1.0, 10.0, 1.0]     # small, unit, large (update clipping kicks in), unit
STAND_IN = ("pytorch_optimizer stand-in (tests/golden/make_golden_came.py): NoSparseGradientError, type aliases, BaseOptimizer with no-op "
            "validate_* and apply_weight_decay = decoupled p.mul_(1 - wd * (1 if fixed_decay else lr)), else grad.add_(p, alpha=wd)")
CASES = [
    ("default", dict(lr=1e-3)),
    ("decay", dict(lr=1e-3, weight_decay=0.01)),
    ("fixed", dict(lr=1e-3, weight_decay=1e-3, fixed_decay=True, clip_threshold=0.5, betas=(0.8, 0.99, 0.999))),
]


def install_pytorch_optimizer_stand_in() -> None:
    class NoSparseGradientError(Exception):
        def __init__(self, optimizer_name: str, note: str = ""):
            super().__init__(f"[-] {optimizer_name} does not support sparse gradient. {note}")

    class BaseOptimizer:
        @staticmethod
        def validate_learning_rate(learning_rate) -> None:
            pass

        @staticmethod
        def validate_betas(betas) -> None:
            pass

        @staticmethod
        def validate_non_negative(x, name) -> None:
            pass

        @staticmethod
        def apply_weight_decay(p, grad, lr, weight_decay, weight_decouple, fixed_decay, ratio=None) -> None:
            if weight_decouple:
                p.mul_(1.0 - weight_decay * (1.0 if fixed_decay else lr) * (ratio if ratio is not None else 1.0))
            elif weight_decay > 0.0 and grad is not None:
                grad.add_(p, alpha=weight_decay)

    mods = {n: types.ModuleType(n) for n in ("pytorch_optimizer", "pytorch_optimizer.base", "pytorch_optimizer.base.exception",
                                             "pytorch_optimizer.base.optimizer", "pytorch_optimizer.base.types")}
    mods["pytorch_optimizer.base.exception"].NoSparseGradientError = NoSparseGradientError
    mods["pytorch_optimizer.base.optimizer"].BaseOptimizer = BaseOptimizer
    t = mods["pytorch_optimizer.base.types"]
    t.BETAS, t.CLOSURE, t.DEFAULTS, t.LOSS, t.PARAMETERS = tuple, object, dict, object, object
    for n in ("pytorch_optimizer", "pytorch_optimizer.base"):
        mods[n].__path__ = []
    sys.modules.update(mods)


def came_case() -> dict:
    """One set of inputs (initial values, four steps of gradients) shared by the three cases and stored once, as bf16: the values are
    rounded to bf16 before the reference sees them, so the bf16 copies are exact and the fixture stays small.  Per case: the
    parameters after every step and the states after the last one, in fp32."""
    from neurosis.optimizers.came import CAME

    sig = inspect.signature(CAME.__init__)
    signature = {k: v.default for k, v in sig.parameters.items() if k not in ("self", "params")}
    g = torch.Generator().manual_seed(4321)
    init = [(torch.randn(*s, generator=g) * (0.5 if len(s) > 1 else 1.0)).bfloat16() for s in SHAPES]
    grads = [[(torch.randn(*s, generator=g) * mag).bfloat16() for s in SHAPES] for mag in GRAD_MAGNITUDES]
    out = {"signature": signature, "shapes": SHAPES, "stand_in": STAND_IN, "init": init, "grads": grads}
    for tag, kw in CASES:
        params = [torch.nn.Parameter(t.float()) for t in init]
        opt = CAME(params, **kw)
        after = []
        for gs in grads:
            for p, gr in zip(params, gs):
                p.grad = gr.float()
            opt.step()
            after.append([p.detach().clone() for p in params])
        states = [{k: v.clone() for k, v in opt.state[p].items()} for p in params]
        out[tag] = dict(kwargs=kw, after=after, states=states, step=int(opt.param_groups[0]["step"]))
        print("came", tag, "|p0| after 4 steps:", float(params[0].detach().norm()))
    return out


if __name__ == "__main__":
    torch.set_num_threads(1)           # one reduction order: the fixture regenerates bit for bit
    install_pytorch_optimizer_stand_in()
    import_reference()
    save_fixture(came_case(), "came_steps")
