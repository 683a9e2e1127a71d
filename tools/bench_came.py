"""The fused CAME update ALONE on the chip, on bench.py's SDXL UNet store (2.57 G parameters), beside the fused Adafactor and AdamW
measured the same way in the same process: ms per update, launches, and effective TB/s over the bytes each touches per parameter
(CAME 34: g read three times, m read twice and written once, p read and written, bf16 shadow written; Adafactor 22; AdamW 30).
Then one short real-step comparison: p50 of 10 training steps (1024^2, batch 4, precomputed text-encoder outputs, hipGraph replay,
the update overlapped with the next step as in bench.py) with CAME and with the default Adafactor.

    usage (GPU box): python tools/bench_came.py"""
import os
import sys
from functools import partial

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from neurosis_amd.optimizers.came import CAME  # noqa: E402

dev = torch.device("cuda", 0)
eng = bench.build_engine(dev, (1024, 1024), None)
n = sum(p.numel() for p in eng.store.params)


def use_adafactor():
    eng._torch_optimizer = None
    eng.configure_adafactor(scale_parameter=True, relative_step=True, warmup_init=True)   # bench.py's default (the example config's)


def use_came():
    eng.adafactor = None
    eng.optimizer = partial(CAME, lr=1e-6, weight_decay=1e-2)
    eng._torch_optimizer = None
    eng.configure_optimizers()


def use_adamw():
    eng.adafactor = None
    eng._torch_optimizer = None


def time_update(reps=5):
    for _ in range(2):
        eng.optimizer_step(lr=1e-6, weight_decay=1e-2, grad_scale=1.0, dp=None)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        eng.optimizer_step(lr=1e-6, weight_decay=1e-2, grad_scale=1.0, dp=None)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


overlap = eng.overlap_optimizer
eng.overlap_optimizer = False                      # in line on the current stream: what is timed is the update itself
eng.store.grad.normal_(0, 1e-3)
results = {}
for name, setup, bpp in (("CAME", use_came, 34), ("Adafactor", use_adafactor, 22), ("AdamW", use_adamw, 30)):
    setup()
    ms = time_update()
    if name == "CAME":
        f = eng._torch_optimizer.flat
        launches = sum(2 + 2 * hm for hm in f._has_matrix)
    elif name == "Adafactor":
        af = eng.adafactor
        launches = sum(2 + int((af._tens_np["kind"][t0:t1] == 1).any()) for (t0, t1, _, _) in af.chunks)
    else:
        launches = 1
    results[name] = ms
    print(f"{name} alone: {ms:.2f} ms per update of {n / 1e9:.3f} G parameters, {launches} launches, "
          f"{bpp * n / ms / 1e9:.2f} TB/s over {bpp} B/param touched")
    if name != "Adafactor":                        # free optimizer state before the next one allocates its own
        eng._torch_optimizer = None
        eng.store.exp_avg = eng.store.exp_avg_sq = None
        torch.cuda.empty_cache()

# -- real steps -------------------------------------------------------------------------------------------------------------------
eng.overlap_optimizer = overlap
gen = torch.Generator(device=dev).manual_seed(42)
B = 4


def train_step():
    batch = bench.synthetic_batch(dev, B, (1024, 1024), gen, True)
    sig = bench.draw_sigmas(B, gen, dev)
    eng.accumulate(0, None, last=True)
    eng.training_step(batch, 0, sigmas=sig).backward()
    eng.optimizer_step(lr=1e-6, weight_decay=1e-2, grad_scale=1.0, dp=None)


def p50_step(steps=10, warm=4):
    for _ in range(warm):                          # graph capture on the second step, then replay
        train_step()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    for i in range(steps):
        marks[i].record()
        train_step()
    marks[steps].record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:]))
    return ts[len(ts) // 2]


use_adafactor()
ms_af = p50_step()
use_came()
ms_came = p50_step()
print(f"real step (1024^2, batch {B}, precomputed TE): CAME p50 {ms_came:.1f} ms = {ms_came / B:.1f} ms/image; "
      f"Adafactor (default) p50 {ms_af:.1f} ms = {ms_af / B:.1f} ms/image")
