"""Cost of training the two CLIP text towers (configs/sdxl/sdxl-te.example.yaml: CLIP-L under layer hidden / 11, bigG under penultimate +
pooled, both trainable) at batch 4 x 77 tokens on one MI355X, piece by piece: the frozen towers' forward (no grad, eager -- what a frozen
step runs when hipGraph replay is off), the training forward (the autograd-connected closure chains), their backward from random
upstream gradients of the conditioner's outputs, and the fused AdamW8bit update over the towers' two flat stores (one parameter group
each, as the engine's groups).  Random weights; p50 of K timed repetitions after W warm-ups, CUDA events around each piece.
--step: the whole sdxl-te training step at 1024^2 instead -- bench.py's engine (frozen VAE encode, UNet fwd + bwd with its gradient of the
conditioning, hipGraph replay) with both towers trainable in its conditioner, AdamW8bit over the three groups under
LegacyCosineAnnealingWarmupRestarts (the config's settings), the update overlapped with the next step as in bench.py: p50 ms per step.

    usage (GPU box): python tools/bench_te_train.py [--step] [--steps K] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from neurosis_amd.models.text_encoder.clip import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder2  # noqa: E402
from neurosis_amd.nn import FlatParamStore  # noqa: E402
from neurosis_amd.optimizers import AdamW8bit  # noqa: E402


def timed(fn, k, w):
    for _ in range(w):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--te-lr", type=float, default=1.0, help="--step: the towers' base_lr (the config's 1.0 is an absolute peak learning rate)")
    a = ap.parse_args()
    if a.step:
        return full_step(a)
    torch.manual_seed(0)
    clip_l = FrozenCLIPEmbedder(device="cuda", layer="hidden", layer_idx=11, is_trainable=True, base_lr=1.0).cuda()
    bigg = FrozenOpenCLIPEmbedder2(device="cuda", layer="penultimate", always_return_pooled=True, is_trainable=True, base_lr=1.0).cuda()
    with torch.no_grad():
        for p in list(clip_l.parameters()) + list(bigg.parameters()):
            if p.dim() >= 2:
                p.normal_(std=p.shape[-1] ** -0.5)
    groups = []
    for name, emb in (("FrozenCLIPEmbedder", clip_l), ("FrozenOpenCLIPEmbedder2", bigg)):
        params = emb.trained_parameters()
        store = FlatParamStore(params)
        store.state.assume_zeroed = False
        groups.append({"name": name, "params": params, "initial_lr": 1.0})
    opt = AdamW8bit(groups, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    B = a.batch
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 49406, (B, 77), generator=g)
    ids[:, 0], ids[:, 20], ids[:, 21:] = 49406, 49407, 0
    ids = ids.cuda()
    up_l = torch.randn(B, 77, 768, generator=g).cuda()
    up_g, up_p = torch.randn(B, 77, 1280, generator=g).cuda(), torch.randn(B, 1280, generator=g).cuda()

    def frozen_forward():
        with torch.no_grad():
            clip_l(ids)
            bigg(ids)

    state = {}

    def train_forward():
        state["outs"] = (clip_l(ids), *bigg(ids))

    def backward():
        torch.autograd.backward(list(state["outs"]), [up_l, up_g, up_p])

    def forward_backward():
        train_forward()
        backward()

    def update():
        opt.step()

    res = {}
    res["frozen_forward_ms"], _ = timed(frozen_forward, a.steps, a.warmup)
    res["train_forward_ms"], _ = timed(train_forward, a.steps, a.warmup)
    bwd = []
    for _ in range(a.warmup + a.steps):
        train_forward()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        backward()
        e1.record()
        torch.cuda.synchronize()
        bwd.append(e0.elapsed_time(e1))
    res["backward_ms"] = statistics.median(bwd[a.warmup:])
    res["forward_backward_ms"], _ = timed(forward_backward, a.steps, a.warmup)
    res["adamw8bit_update_ms"], _ = timed(update, a.steps, a.warmup)
    res["trained_parameters"] = sum(p.numel() for gr in groups for p in gr["params"])
    res["batch"] = B
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def full_step(a):
    from functools import partial

    import bench
    from neurosis_amd.modules.encoders import ConcatTimestepEmbedderND, GeneralConditioner
    from neurosis_amd.schedulers import LegacyCosineAnnealingWarmupRestarts

    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    embedders = [FrozenCLIPEmbedder(layer="hidden", layer_idx=11, input_key="caption_ids", device=dev, is_trainable=True, base_lr=a.te_lr),
                 FrozenOpenCLIPEmbedder2(arch="ViT-bigG-14", version=None, layer="penultimate", always_return_pooled=True, legacy=False,
                                         input_key="caption_ids", device=dev, is_trainable=True, base_lr=a.te_lr)]
    embedders += [ConcatTimestepEmbedderND(outdim=256, input_key=k) for k in ("original_size_as_tuple", "crop_coords_top_left", "target_size_as_tuple")]
    eng = bench.build_engine(dev, (1024, 1024), GeneralConditioner(embedders).to(dev))
    eng.optimizer = partial(AdamW8bit, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    eng.scheduler = partial(LegacyCosineAnnealingWarmupRestarts, first_cycle_steps=50, cycle_mult=1.0, min_lr=3e-7, warm_up_steps=25, gamma=0.9)
    eng.configure_optimizers()
    gen = torch.Generator(device=dev).manual_seed(0)
    B = a.batch
    events, losses = [], []
    for i in range(a.warmup + a.steps):
        batch = bench.synthetic_batch(dev, B, (1024, 1024), gen, precomputed_te=False)
        sig = bench.draw_sigmas(B, gen, dev)
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = eng.training_step(batch, 0, sigmas=sig)
        loss.backward()
        eng.optimizer_step()
        losses.append(loss.detach())
        events.append(e0)
        if i < a.warmup:
            torch.cuda.synchronize()
    end = torch.cuda.Event(enable_timing=True)
    eng.join_optimizer()
    end.record()
    torch.cuda.synchronize()
    events.append(end)
    times = [events[i].elapsed_time(events[i + 1]) for i in range(len(events) - 1)]     # start to start, no host sync in between
    res = {"sdxl_te_step_ms_p50": round(statistics.median(times[a.warmup:]), 2), "sdxl_te_step_ms_min": round(min(times[a.warmup:]), 2),
           "te_base_lr": a.te_lr, "losses": [round(float(l), 4) for l in losses], "groups": [g["name"] for g in eng._torch_optimizer.param_groups],
           "trained_parameters": [sum(p.numel() for p in g["params"]) for g in eng._torch_optimizer.param_groups], "batch": B,
           "max_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
