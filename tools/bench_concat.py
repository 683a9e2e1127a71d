"""Step time of a concat-conditioned SDXL UNet (in_channels = 9: an inpainting model's mask + masked-image latents behind the latents)
at the benchmark's shape -- 1024^2, batch 4, frozen VAE encode, UNet forward + backward, fused Adafactor; synthetic weights and
synthetic text-encoder outputs.  bench.py measures the text-to-image model and is not touched by this.

    python tools/bench_concat.py [--steps 20] [--warmup 3] [--tree DIR]        one run: a JSON line with the step times
    python tools/bench_concat.py --ab DIR [--rounds 2]                         this checkout against the one at DIR, alternating

--tree DIR imports the package from another checkout (built there), e.g. the commit before concat conditioning stayed on the fused
path, where such a model takes the generic route (Denoiser.forward -> torch.cat -> UNetModel.forward, the chain launched eagerly).
Whole steps are timed with device events after the warm-up (and after the two priming steps that capture the hipGraphs); p50 over --steps.
As tools/ab_bench.py: every run is a fresh process, the variants interleaved round by round so that drift cancels."""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--tree", default=None)
ap.add_argument("--ab", default=None)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--timeout", type=int, default=600, help="seconds one run of --ab may take")
a = ap.parse_args()
here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if a.ab is not None:
    res = {"this": [], "other": []}
    for rnd in range(a.rounds):
        for name, tree in (("other", a.ab), ("this", here)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--batch", str(a.batch),
                                "--res", str(a.res), "--tree", tree], capture_output=True, text=True, timeout=a.timeout)
            line = next((l for l in p.stdout.splitlines() if l.startswith("{")), None)
            if line is None:
                print(f"{name}: FAILED rc={p.returncode}\n{p.stderr[-1500:]}", flush=True)
                sys.exit(1)           # (nothing more is started on the GPU after a failed run)
            o = json.loads(line)
            res[name].append(o)
            print(f"round {rnd} {name:6s} route {o['route']:8s} p50 {o['step_ms_p50']:8.2f}  mean {o['ms_per_step']:8.2f}  loss {o['loss']:.5f}", flush=True)
    print(json.dumps({k: {"route": v[0]["route"], "step_ms_p50": [o["step_ms_p50"] for o in v], "ms_per_step": [o["ms_per_step"] for o in v]} for k, v in res.items()}))
    sys.exit(0)

sys.path.insert(0, os.path.abspath(a.tree or here))
import torch  # noqa: E402

import neurosis_amd.modules.diffusion as D  # noqa: E402
from neurosis_amd import lib  # noqa: E402
from neurosis_amd.models.autoencoder import AutoencoderKL  # noqa: E402
from neurosis_amd.models.diffusion import DiffusionEngine  # noqa: E402

SDXL_UNET = dict(adm_in_channels=2816, num_classes="sequential", use_checkpoint=False, in_channels=9, out_channels=4, model_channels=320,
                 attention_resolutions=[4, 2], num_res_blocks=2, channel_mult=[1, 2, 4], num_head_channels=64, use_linear_in_transformer=True,
                 transformer_depth=[1, 2, 10], context_dim=2048, spatial_transformer_attn_type="softmax-xformers")
SDXL_VAE_DD = dict(attn_type="vanilla-xformers", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                   num_res_blocks=2, attn_resolutions=[], dropout=0.0)

lib.load()
device = torch.device("cuda", 0)
torch.manual_seed(42)
with torch.device(device):
    unet = D.UNetModel(**SDXL_UNET)
    vae = AutoencoderKL(embed_dim=4, ddconfig=SDXL_VAE_DD)
    denoiser = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization())
g = torch.Generator(device=device).manual_seed(0)
with torch.no_grad():          # zero_module()-initialised layers get values, so that gradients are non-trivial
    for p in unet.parameters():
        if p.dim() > 1 and float(p.abs().max()) == 0.0:
            p.copy_(torch.randn(p.shape, generator=g, device=device) * 0.02)
loss_fn = D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())
# (no conditioner: the engine's stand-in hands on the "crossattn" / "vector" / "concat" entries the batch carries)
eng = DiffusionEngine(model=unet, denoiser=denoiser.to(device), first_stage_model=vae, loss_fn=loss_fn, scale_factor=0.13025, input_key="image")
eng.setup_flat_params()
eng.configure_adafactor(scale_parameter=True, relative_step=True, warmup_init=True)

routes = []
fused_unet = D.OpenAIWrapper.fused_unet


def noting_the_route(self, *args, **kw):
    unet = fused_unet(self, *args, **kw)
    routes.append(unet is not None)
    return unet


D.OpenAIWrapper.fused_unet = noting_the_route
gen = torch.Generator(device=device).manual_seed(42)
h = a.res // 8


def step():
    mask = (torch.rand(a.batch, 1, h, h, device=device, generator=gen) > 0.5).float()
    batch = {"image": torch.rand(a.batch, 3, a.res, a.res, device=device, generator=gen) * 2 - 1,
             "crossattn": torch.randn(a.batch, 77, 2048, device=device, generator=gen), "vector": torch.randn(a.batch, 2816, device=device, generator=gen),
             "concat": torch.cat((mask, torch.randn(a.batch, 4, h, h, device=device, generator=gen) * (1.0 - mask)), 1)}
    sig = (-1.2 + 1.2 * torch.randn(a.batch, device=device, generator=gen)).exp().clamp(0.0292, 14.61)
    loss = eng.training_step(batch, 0, sigmas=sig)
    loss.backward()
    eng.optimizer_step(lr=1e-6, weight_decay=1e-2)
    return loss


for _ in range(2 + a.warmup):         # two priming steps (the second captures the hipGraphs where the chain is replayed), then the warm-up
    step()
torch.cuda.synchronize()
marks = []
for _ in range(a.steps):
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    marks.append(ev)
    loss = step()
ev = torch.cuda.Event(enable_timing=True)
ev.record()
marks.append(ev)
eng.join_optimizer()
torch.cuda.synchronize()
ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps))
assert len(set(routes)) == 1
print(json.dumps({"route": "fused" if routes[0] else "generic", "step_ms_p50": round(ms[len(ms) // 2], 3), "ms_per_step": round(marks[0].elapsed_time(marks[-1]) / a.steps, 3),
                  "step_ms_min": round(ms[0], 3), "steps": a.steps, "batch": a.batch, "res": a.res, "loss": float(loss), "device": torch.cuda.get_device_name(0)}))
