"""One informational number for the ADM block family: the training step (forward, backward, fused AdamW) of a 320-wide, three-level
UNet built from scale-shift ResBlocks with resblock_updown, 64 x 64 latents, batch 4.  Not the project's metric (that is bench.py).

usage: python tools/bench_adm.py [--steps 10] [--warmup 4] [--batch 4] [--plain]
--plain: the same network with use_scale_shift_norm=False, resblock_updown=False (the SD-style blocks), for comparison.
Under `rocprofv3 --kernel-trace -- python tools/bench_adm.py ...` followed by tools/kstats.py the per-kernel shares come out; the new
kernels are gn_apply_kernel<true>, gn_bwd_stats_kernel<true>, gn_bwd_apply_kernel<true>, colpart_reduce_mod_kernel, gn_dmod_kernel,
nk_ew_pixels_kernel<AvgPool2xFwd>, <AvgPool2xBwd> and <Up2Fwd>."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import neurosis_amd.modules.diffusion as D  # noqa: E402
from neurosis_amd.nn import FlatParamStore  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--plain", action="store_true")
a = ap.parse_args()

cfg = dict(in_channels=4, model_channels=320, out_channels=4, num_res_blocks=2, attention_resolutions=[2, 4], channel_mult=[1, 2, 4], num_head_channels=64,
           transformer_depth=1, context_dim=768, use_linear_in_transformer=True, num_classes="sequential", adm_in_channels=512,
           use_scale_shift_norm=not a.plain, resblock_updown=not a.plain)
torch.manual_seed(0)
net = D.UNetModel(**cfg)
with torch.no_grad():       # the reference zero-initialises every block's last convolution: give them weights so the backward is a real one
    for k, p in net.named_parameters():
        if k.endswith(("out_layers.3.weight", "proj_out.weight", "out.2.weight")):
            p.normal_(0.0, 0.02)
net = net.cuda()
store = FlatParamStore(net.parameters())
store.state.wgrad_stream = torch.cuda.Stream()
den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization()).cuda()
lossfn = D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())
wrapped = D.OpenAIWrapper(net)
g = torch.Generator().manual_seed(1)
B = a.batch
x, noise = torch.randn(B, 4, 64, 64, generator=g).cuda(), torch.randn(B, 4, 64, 64, generator=g).cuda()
cond = {"crossattn": torch.randn(B, 77, 768, generator=g).cuda(), "vector": torch.randn(B, 512, generator=g).cuda()}
sigma = (torch.rand(B, generator=g) * 5 + 0.1).cuda()

times, loss = [], None
for i in range(a.warmup + a.steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = lossfn._forward(wrapped, den, cond, x, {}, sigmas=sigma, noise=noise)
    loss.mean().backward()
    store.adamw_step(1e-5, (0.9, 0.999), 1e-8, 0.0, 1.0)
    torch.cuda.synchronize()
    if i >= a.warmup:
        times.append((time.perf_counter() - t0) * 1e3)
print(json.dumps(dict(config="adm-320x3-ssn-updown" if not a.plain else "plain-320x3", batch=B, latents=64, params=sum(p.numel() for p in net.parameters()),
                      steps=a.steps, ms_per_step=round(sum(times) / len(times), 3), step_ms_p50=round(statistics.median(times), 3),
                      step_ms_min=round(min(times), 3), loss=[round(float(v), 5) for v in loss.detach().float().cpu()])))
