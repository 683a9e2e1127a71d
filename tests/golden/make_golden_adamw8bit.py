#!/usr/bin/env python
"""Generates tests/golden/adamw8bit_steps.{json,safetensors}: four steps of 8-bit blockwise AdamW (bitsandbytes' AdamW8bit algorithm,
as defined in neurosis_amd/optim.py FlatAdamW8bit) from the pure-torch CPU restatement in THIS file, on a mixed parameter set.

    python tests/golden/make_golden_adamw8bit.py

bitsandbytes is not a dependency, so the fixture pins the algorithm as restated here, not bitsandbytes' own kernels; bit-for-bit
interchange with bitsandbytes is not claimed.  The restatement works in fp32 with every element-wise operation rounded once -- the
order the HIP kernel uses -- and the scalars rounded to fp32 as the host passes them; `restated_step(..., dtype=torch.float64)` is the
fp64 variant the GPU tests compare larger shapes against.

Inputs (initial values and every step's gradients) are bf16-exact and shared by the two cases; they are stored once, as bf16.  The
parameter set, kept small (the fixture is about 0.4 MB): a 2-D matrix and a 4-D conv weight above min_8bit_size whose lengths are not
multiples of 256 (the matrix's last block holds 5 elements, so one lane holds a single one), tensors below min_8bit_size (fp32 state), and
one block of the matrix whose gradient is zero at every step (absmax 0, the code of 0.0).  Per case: the parameters after every step
(fp32), and after the last step the codes / fp32 moments and the absmax of every block.
"""
from __future__ import annotations

import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from tests.golden.fixture_io import save_fixture  # noqa: E402

A8_BLOCK = 256
MIN_8BIT_SIZE = 4096
SHAPES = [(3, 1367), (29, 16, 3, 3), (320,), (8, 8, 3, 3), (7,)]
GRAD_MAGNITUDES = [1e-3, 1e-2, 1.0, 1e-1]
ZERO_BLOCK = (0, 1)            # parameter 0, block 1 (elements 256..511): zero gradient at every step
CASES = [
    ("sdxl_te", dict(lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)),    # the reference's configs/sdxl/sdxl-te.example.yaml
    ("decay", dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05)),
]


def dynamic_map(signed: bool) -> torch.Tensor:
    """bitsandbytes' create_dynamic_map(signed, max_exponent_bits=7, total_bits=8), restated."""
    data = []
    for i in range(7):
        n = 2 ** i if signed else 2 ** (i + 1)
        b = torch.linspace(0.1, 1, n + 1)
        means = ((b[:-1] + b[1:]) / 2.0).tolist()
        data += [10 ** (i - 6) * x for x in means]
        if signed:
            data += [-(10 ** (i - 6)) * x for x in means]
    data += [0.0, 1.0]
    return torch.tensor(sorted(data), dtype=torch.float32)


def phys(t: torch.Tensor) -> torch.Tensor:
    """A parameter's elements in the flat store's physical order (conv weights [O][KH][KW][I])."""
    return (t.permute(0, 2, 3, 1) if t.dim() == 4 else t).reshape(-1)


def unphys(flat: torch.Tensor, shape) -> torch.Tensor:
    if len(shape) == 4:
        O, I, KH, KW = shape
        return flat.reshape(O, KH, KW, I).permute(0, 3, 1, 2).contiguous()
    return flat.reshape(shape)


def nearest(q: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """argmin_i |q[i] - x| with the lowest index on a tie, for sorted q.  Computed from the two neighbours of x (searchsorted): the rounded
    distance is monotone on either side of x, so this is the argmin over all 256 entries (test_adamw8bit_cpu checks it against the
    brute-force argmin)."""
    pos = torch.searchsorted(q, x, right=True)              # #{i : q[i] <= x}
    lo, hi = (pos - 1).clamp(0, 255), pos.clamp(0, 255)
    return torch.where((x - q[lo]).abs() <= (q[hi] - x).abs(), lo, hi).to(torch.uint8)


def blockwise_absmax(x: torch.Tensor) -> torch.Tensor:
    n = x.numel()
    pad = torch.zeros(-(-n // A8_BLOCK) * A8_BLOCK, dtype=x.dtype)
    pad[:n] = x.abs()
    return pad.view(-1, A8_BLOCK).amax(dim=1)


def init_state(numel: int, dtype=torch.float32, min_8bit_size: int = MIN_8BIT_SIZE) -> dict:
    """Step-0 state of one parameter (flat, physical order): codes of 0.0 and absmax 0, or fp32 zeros for a small parameter."""
    if numel < min_8bit_size:
        return {"state1": torch.zeros(numel, dtype=dtype), "state2": torch.zeros(numel, dtype=dtype)}
    q1, q2 = dynamic_map(True), dynamic_map(False)
    nb = -(-numel // A8_BLOCK)
    return {"state1": torch.full((numel,), int((q1 == 0).nonzero()[0]), dtype=torch.uint8),
            "state2": torch.full((numel,), int((q2 == 0).nonzero()[0]), dtype=torch.uint8),
            "absmax1": torch.zeros(nb, dtype=dtype), "absmax2": torch.zeros(nb, dtype=dtype)}


def restated_step(p: torch.Tensor, g: torch.Tensor, st: dict, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                  weight_decay: float = 1e-2, grad_scale: float = 1.0, dtype=torch.float32) -> torch.Tensor:
    """One AdamW8bit step of one parameter, given and returned flat in physical order; `st` (init_state) is updated in place.
    fp32: every operation rounds once and the scalars are the fp32 values the host passes the kernel (1 - beta, 1 - lr wd and the bias
    corrections computed in double first).  fp64: the same arithmetic in double."""
    def s(x):                                    # a host scalar as the arithmetic sees it
        return torch.tensor(x, dtype=dtype)

    b1, b2 = betas
    B1, B2, OMB1, OMB2 = s(b1), s(b2), s(1.0 - b1), s(1.0 - b2)
    BC1, BC2, DECAY = s(1.0 - b1 ** step), s(1.0 - b2 ** step), s(1.0 - lr * weight_decay)
    LR, EPS, GS = s(lr), s(eps), s(grad_scale)
    p, g = p.to(dtype), g.to(dtype) * GS
    q8 = "absmax1" in st
    n = p.numel()
    if q8:
        q1, q2 = dynamic_map(True).to(dtype), dynamic_map(False).to(dtype)
        blk = torch.arange(n) // A8_BLOCK
        m = q1[st["state1"].long()] * st["absmax1"].to(dtype)[blk]
        v = q2[st["state2"].long()] * st["absmax2"].to(dtype)[blk]
    else:
        m, v = st["state1"].to(dtype), st["state2"].to(dtype)
    m = B1 * m + OMB1 * g
    v = B2 * v + OMB2 * (g * g)
    p = p * DECAY - LR * ((m / BC1) / (torch.sqrt(v / BC2) + EPS))
    if q8:
        for k, x, q in (("1", m, q1), ("2", v, q2)):
            am = blockwise_absmax(x)
            ame = am[blk]
            st["absmax" + k] = am
            st["state" + k] = nearest(q, torch.where(ame > 0, x / torch.where(ame > 0, ame, 1), torch.zeros_like(x)))
    else:
        st["state1"], st["state2"] = m, v
    return p


def adamw8bit_case() -> dict:
    g = torch.Generator().manual_seed(8080)
    init = [(torch.randn(*s, generator=g) * (0.5 if len(s) > 1 else 1.0)).bfloat16() for s in SHAPES]
    grads = []
    for mag in GRAD_MAGNITUDES:
        gs = [(torch.randn(*s, generator=g) * mag).bfloat16() for s in SHAPES]
        ti, b = ZERO_BLOCK
        gs[ti].view(-1)[b * A8_BLOCK:(b + 1) * A8_BLOCK] = 0
        grads.append(gs)
    out = {"shapes": SHAPES, "min_8bit_size": MIN_8BIT_SIZE, "block": A8_BLOCK, "zero_block": ZERO_BLOCK, "qmap1": dynamic_map(True),
           "qmap2": dynamic_map(False), "init": init, "grads": grads}
    for tag, kw in CASES:
        params = [phys(t.float()) for t in init]
        states = [init_state(p.numel()) for p in params]
        after = []
        for step, gs in enumerate(grads, 1):
            params = [restated_step(p, phys(gr.float()), st, step, **kw) for p, gr, st in zip(params, gs, states)]
            after.append([unphys(p, s) for p, s in zip(params, SHAPES)])
        finals = [{k: (unphys(v, shape) if k.startswith("state") else v) for k, v in st.items()} for st, shape in zip(states, SHAPES)]
        out[tag] = dict(kwargs=kw, after=after, states=finals, step=len(grads))
        print("adamw8bit", tag, "|p0| after 4 steps:", float(params[0].norm()))
    return out


if __name__ == "__main__":
    torch.set_num_threads(1)           # one reduction order: the fixture regenerates bit for bit
    save_fixture(adamw8bit_case(), "adamw8bit_steps")
