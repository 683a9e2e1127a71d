"""Fixture of the DreamSim loss: the reference's own VisionTransformer run on the CPU in float64.

    python -m tests.golden.make_golden_dreamsim        ->  tests/golden/dreamsim_tiny.{json,safetensors}

The reference's `vit.py` and `common.py` are loaded by file path (the package's __init__ pulls in diffusers, which is not installed); the
ensemble around them -- Normalize, the three towers side by side, z = f / |f| - mean, d = 1 - cos -- is model.py:153-172 and :27-31 restated,
and the loss-level pipeline (clamp to [-1, 1], x / 2 + 0.5 with its clamp) is autoencoding/losses/dreamsim.py:114-125.

Towers: the three ensemble variants (dino: no pre-norm, GELU, eps 1e-6, no final norm, no head; clip1 / clip2: pre-norm, quick-GELU / GELU,
eps 1e-5, final norm, head) at embed_dim 128, 2 heads, depth 2, patch 16, img_size 32, head width 16.  Weights are seeded and scaled by
fan-in (the default 0.02 init gives embeddings that barely depend on the image); they are rebuilt from their names by
tests/dreamsim_fixture.py, and the fixture holds their shapes and checksums only.  Inputs: B = 3 images at 32 x 32 (5 tokens) and at 48 x 48
(10 tokens, through the interpolated position table); recons = clamp(x + 0.25 noise).

Recorded, float64 rounded to fp32: per-tower embeddings of both images, d [B], d(sum d) / d recons, the interpolated position tables; the
same under torch.autocast("cpu", bfloat16) of an fp32 copy as DEVIATIONS from the float64 run (max |a - b| / max |b|, and the cosine): what
bf16 compute costs the reference itself, the yardstick of the GPU tests.  Also ViT-B's state-dict keys / shapes and constructor argument
names.  Every recorded d is asserted >= 0.05: 1 - cos is ill-conditioned below that.
"""
from __future__ import annotations

import copy
import importlib.util
import inspect
import sys
import types
from functools import partial

import torch
import torch.nn.functional as F

from tests.dreamsim_fixture import HEAD_WIDTH, PATCH, TINY, checksums, seeded_state
from tests.golden.fixture_io import save_fixture
from tests.golden.make_golden import REF_SRC

B = 3
SIZES = (32, 48)
TOWERS = (("dino", dict(pre_norm=False, act_layer="gelu", layer_norm_eps=1e-6, num_classes=0), False),
          ("clip1", dict(pre_norm=True, act_layer="quick_gelu", layer_norm_eps=1e-5, num_classes=HEAD_WIDTH), True),
          ("clip2", dict(pre_norm=True, act_layer="gelu", layer_norm_eps=1e-5, num_classes=HEAD_WIDTH), True))
DINO_NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
CLIP_NORM = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))


def load_reference_vit():
    """the reference's dreamsim/common.py and vit.py as a two-module package, without its __init__"""
    root = REF_SRC / "neurosis" / "modules" / "losses" / "dreamsim"
    pkg = types.ModuleType("_ref_dreamsim")
    pkg.__path__ = [str(root)]
    sys.modules["_ref_dreamsim"] = pkg
    mods = {}
    for name in ("common", "vit"):
        spec = importlib.util.spec_from_file_location(f"_ref_dreamsim.{name}", root / f"{name}.py")
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["vit"]


def normalize(x, stats):
    mean, std = (torch.tensor(s, dtype=x.dtype).view(1, 3, 1, 1) for s in stats)
    return (x - mean) / std


def ensemble(towers: dict, inputs, recons):
    """(per-tower embeddings {name: [2B, w]}, d [B]) of the loss-level pipeline"""
    x = torch.cat(((inputs.clamp(-1, 1) / 2 + 0.5).clamp(0, 1), (recons.clamp(-1, 1) / 2 + 0.5).clamp(0, 1)), dim=0)
    emb = {}
    for name, _, norm in TOWERS:
        emb[name] = towers[name](normalize(x, DINO_NORM if name == "dino" else CLIP_NORM), norm=norm)
    z = torch.cat([emb[name] for name, _, _ in TOWERS], dim=1)
    z = z.div(z.norm(dim=1, keepdim=True))
    z = z.sub(z.mean(dim=1, keepdim=True)).view(2, inputs.shape[0], -1)
    return emb, 1 - F.cosine_similarity(z[0], z[1], dim=1)


def deviation(got, want) -> dict:
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    return {"rel": float((got - want).abs().max() / want.abs().max()), "cosine": float(torch.dot(got, want) / (got.norm() * want.norm()))}


SEED = 20241021          # of the images and the noise (the first from 20241020 on at which every d clears the 0.05 asserted below); the weights are tests/dreamsim_fixture.py's


def main(seed: int = SEED) -> None:
    vit = load_reference_vit()
    g = torch.Generator().manual_seed(seed)
    towers32, state = {}, {}
    for name, kw, _ in TOWERS:      # vit_base_dreamsim fixes embed_dim / depth / num_heads at ViT-B's: the tiny shape goes to the class it calls
        kw = dict(kw)
        act = vit.get_act_layer(kw.pop("act_layer"))
        eps = kw.pop("layer_norm_eps")
        t = vit.VisionTransformer(patch_size=PATCH, mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=eps), act_layer=act, **kw, **TINY)
        sd = seeded_state({f"{name}.{k}": v.shape for k, v in t.state_dict().items()})
        t.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items()})
        towers32[name] = t.eval().requires_grad_(False)
        state.update(sd)
    towers64 = {name: copy.deepcopy(t).double() for name, t in towers32.items()}

    out = {"vit_config": TINY, "num_classes": [0, HEAD_WIDTH, HEAD_WIDTH], "patch_size": PATCH,
           "state_shapes": {k: list(v.shape) for k, v in state.items()}, "state_checksums": checksums(state), "cases": {}}
    for size in SIZES:
        x = 1.05 * (torch.rand(B, 3, size, size, generator=g) * 2 - 1)          # (a few pixels leave [-1, 1]: the loss clamps them)
        recons = (x + 0.25 * torch.randn(x.shape, generator=g)).clamp(-1, 1)
        r64 = recons.double().requires_grad_(True)
        emb64, d64 = ensemble(towers64, x.double(), r64)
        (grad64,) = torch.autograd.grad(d64.sum(), r64)
        assert float(d64.detach().min()) >= 0.05, d64
        r32 = recons.clone().requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            emb_ac, d_ac = ensemble(towers32, x, r32)
        (grad_ac,) = torch.autograd.grad(d_ac.float().sum(), r32)
        pos = {}
        for name in towers64:
            tokens = torch.zeros(1, 1 + (size // PATCH) ** 2, TINY["embed_dim"], dtype=torch.float64)
            pos[name] = towers64[name].interpolate_pos_encoding(tokens, size, size)[0].float()
        out["cases"][str(size)] = {
            "inputs": x, "recons": recons.detach(), "emb": {k: v.detach().float() for k, v in emb64.items()}, "d": d64.detach().float(),
            "grad": grad64.float(), "pos": pos,
            "autocast": {"d": deviation(d_ac.detach(), d64.detach()), "grad": deviation(grad_ac, grad64),
                         "emb": {k: deviation(emb_ac[k].detach(), emb64[k].detach()) for k in emb64}},
        }
        print(size, "d", d64.tolist(), "autocast d", out["cases"][str(size)]["autocast"]["d"], "grad", out["cases"][str(size)]["autocast"]["grad"])

    base = vit.vit_base_dreamsim(num_classes=512, pre_norm=True, act_layer="quick_gelu")
    out["vit_b_clip_keys"] = {k: list(v.shape) for k, v in base.state_dict().items()}
    out["vit_b_dino_keys"] = {k: list(v.shape) for k, v in vit.vit_base_dreamsim(num_classes=0).state_dict().items()}
    out["vit_args"] = {k: (p.default if isinstance(p.default, (int, float, bool, str)) else None)
                       for k, p in inspect.signature(vit.VisionTransformer.__init__).parameters.items() if k not in ("self", "kwargs")}
    out["vit_base_args"] = [k for k in inspect.signature(vit.vit_base_dreamsim).parameters if k != "kwargs"]
    save_fixture(out, "dreamsim_tiny")


if __name__ == "__main__":
    main()
