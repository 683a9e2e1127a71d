#!/usr/bin/env python
"""Generates tests/golden/adafactor_beta1_steps.{safetensors,json}: three steps of the REFERENCE's Adafactor (optimizers/adafactor.py) with
its first moment, beta1 = 0.9, on the CPU, over the parameter set of make_golden.py::adafactor_case (matrices, 3x3 and 1x1 conv weights
(OIHW), vectors), imported through the same stand-in modules.  Two hyper-parameter sets: the relative step with scale_parameter, and a
manual lr with weight decay.  Inputs: initial values and per-step gradients; outputs: the parameters after every step, and `exp_avg` and
the factored states after the last one.  No pickle (fixture_io.py).

    python tests/golden/make_golden_adafactor_beta1.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from tests.golden.fixture_io import save_fixture  # noqa: E402
from tests.golden.make_golden import import_reference  # noqa: E402

BETA1 = 0.9
SHAPES = [(48, 32), (40, 64), (300, 8), (16, 8, 3, 3), (8, 16, 1, 1), (32,), (7,), (1200,)]      # adafactor_case()'s
CASES = [("relative", dict(scale_parameter=True, relative_step=True, warmup_init=False)),
         ("manual", dict(lr=1e-3, scale_parameter=False, relative_step=False, weight_decay=0.01))]


def adafactor_beta1_case():
    from neurosis.optimizers.adafactor import Adafactor

    g = torch.Generator().manual_seed(4321)
    out = {}
    for tag, kw in CASES:
        kw = dict(kw, beta1=BETA1)
        params = [torch.nn.Parameter(torch.randn(*s, generator=g) * (0.5 if len(s) > 1 else 1.0)) for s in SHAPES]
        init = [p.detach().clone() for p in params]
        opt = Adafactor(params, **kw)
        grads, after = [], []
        for step in range(3):
            gs = [torch.randn(*s, generator=g) * (10.0 ** (step - 1)) for s in SHAPES]   # small, unit, large: clipping kicks in
            for p, gr in zip(params, gs):
                p.grad = gr.clone()
            opt.step()
            grads.append(gs)
            after.append([p.detach().clone() for p in params])
        states = []
        for p in params:
            st = opt.state[p]
            assert "exp_avg" in st
            states.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()})
        out[tag] = dict(kwargs=kw, shapes=SHAPES, init=init, grads=grads, after=after, states=states)
        print("adafactor beta1", tag, "lr of p0 after 3 steps:", opt._get_lr(opt.param_groups[0], opt.state[params[0]]))
    save_fixture(out, "adafactor_beta1_steps")


if __name__ == "__main__":
    import_reference()
    adafactor_beta1_case()
