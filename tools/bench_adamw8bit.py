"""The fused 8-bit blockwise AdamW update (AdamW8bit) ALONE on the chip, on bench.py's SDXL UNet store (2.57 G parameters), beside the
fused AdamW and Adafactor measured the same way in the same process: ms per update, launches, and effective TB/s over the bytes each
touches per parameter (AdamW8bit 18: p read and written, g read, the two codes read and written, bf16 shadow written -- the absmax and
the small tensors' fp32 moments add well under 1 %; AdamW 30; Adafactor 22), and the optimizer state in GB.  Then one short real-step
comparison: p50 of 10 training steps (1024^2, batch 4, precomputed text-encoder outputs, hipGraph replay, the update overlapped with the
next step as in bench.py) with AdamW8bit and with the default Adafactor.

    usage (GPU box): python tools/bench_adamw8bit.py"""
import os
import sys
from functools import partial

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from neurosis_amd.optimizers import AdamW8bit  # noqa: E402

dev = torch.device("cuda", 0)
eng = bench.build_engine(dev, (1024, 1024), None)
n = sum(p.numel() for p in eng.store.params)


def use_adafactor():
    eng._torch_optimizer = None
    eng.configure_adafactor(scale_parameter=True, relative_step=True, warmup_init=True)   # bench.py's default (the example config's)


def use_adamw8bit():
    eng.adafactor = None
    eng.optimizer = partial(AdamW8bit, lr=1e-6, weight_decay=1e-2)
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
for name, setup, bpp in (("AdamW8bit", use_adamw8bit, 18), ("AdamW", use_adamw, 30), ("Adafactor", use_adafactor, 22)):
    setup()
    ms = time_update()
    if name == "AdamW8bit":
        f = eng._torch_optimizer.flat
        launches = 1
        state = sum(t.numel() * t.element_size() for t in (f.code1, f.code2, f.absmax1, f.absmax2, f.m32, f.v32))
        print(f"AdamW8bit state: {state / 1e9:.2f} GB = {state / n:.3f} B/param ({int(f._tens_np['is8'].sum())} of {f.ntensors} tensors 8-bit, "
              f"{f.nblocks} blocks); AdamW's fp32 m, v: {8 * n / 1e9:.2f} GB")
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
use_adamw8bit()
ms_8 = p50_step()
print(f"real step (1024^2, batch {B}, precomputed TE): AdamW8bit p50 {ms_8:.1f} ms = {ms_8 / B:.1f} ms/image; "
      f"Adafactor (default) p50 {ms_af:.1f} ms = {ms_af / B:.1f} ms/image")
