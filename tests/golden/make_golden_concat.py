"""Golden fixture for concat-conditioned UNets (inpainting / edit / upscale models: extra input channels joined to the latents by
OpenAIWrapper.forward).  Run from the repository root on a machine that has the reference checkout (CPU only):

    python -m tests.golden.make_golden_concat

Writes concat_tiny.{safetensors,json} (data only) from the reference's own UNetModel(in_channels=9), OpenAIWrapper, DiscreteDenoiser / Denoiser,
StandardDiffusionLoss._forward and VanillaCFG:

  cases/edm_l2, cases/rf_l2   per-sample loss, the sampled gradients (GRAD_KEYS) and every gradient norm, as loss_class_tiny stores them (a
                              gradient of more than GRAD_WHOLE_MAX elements as its first GRAD_ROWS rows: its norm pins the rest), for
                              latents (2, 4, 16, 24) with a (2, 5, 16, 24) concat entry: channel 0 a 0/1 mask, channels 1-4 the latents of
                              another image outside the mask (unit-variance values, the size of c_in * z_t, so that the first convolution's
                              gradient over those columns is as well conditioned as over the latent columns)
  sample                      one classifier-free-guided denoiser evaluation, guider(denoiser(*guider.prepare_inputs(x, sigma, c, uc)), sigma),
                              with DIFFERENT concat tensors in c and uc
"""
from __future__ import annotations

import torch

from tests.golden.fixture_io import save_fixture
from tests.golden.make_golden import GRAD_KEYS, UNET_TINY, FixedSigma, import_reference, synth_state_dict

UNET_CONCAT_TINY = dict(UNET_TINY, in_channels=9)
CONCAT_SHAPE = (2, 4, 16, 24)          # the latents; the concat entry has 5 channels
CONCAT_CASES = [("edm_l2", dict(loss_type="l2", objective_type="edm")), ("rf_l2", dict(loss_type="l2", objective_type="rf"))]
SEED = 4343
CFG_SCALE = 5.0
GRAD_WHOLE_MAX = 65536
GRAD_ROWS = 16


def grad_rows(g: torch.Tensor) -> torch.Tensor:
    """a gradient as the fixture stores it (the test slices the HIP path's gradient the same way)"""
    return (g if g.numel() <= GRAD_WHOLE_MAX else g[:GRAD_ROWS]).contiguous()


def block_mask(g: torch.Generator, B: int, H: int, W: int) -> torch.Tensor:
    """a 0/1 mask [B, 1, H, W] made of 4 x 4 blocks (about half of them set)"""
    coarse = (torch.rand(B, 1, H // 4, W // 4, generator=g) > 0.5).float()
    return coarse.repeat_interleave(4, 2).repeat_interleave(4, 3)


def concat_entry(g: torch.Generator) -> torch.Tensor:
    B, C, H, W = CONCAT_SHAPE
    mask = block_mask(g, B, H, W)
    other = torch.randn(B, C, H, W, generator=g)
    return torch.cat((mask, other * (1.0 - mask)), 1)


def concat_case(nd):
    from neurosis.modules.diffusion.loss import StandardDiffusionLoss
    from neurosis.modules.guidance import VanillaCFG

    cfg = UNET_CONCAT_TINY
    torch.manual_seed(0)
    net = nd.UNetModel(**cfg).eval()
    shapes = {k: list(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict(synth_state_dict(shapes))
    wrapper = nd.OpenAIWrapper(net)
    g = torch.Generator().manual_seed(78)
    B = CONCAT_SHAPE[0]
    x = torch.randn(CONCAT_SHAPE, generator=g)
    ctx = torch.randn(B, 7, cfg["context_dim"], generator=g)
    y = torch.randn(B, cfg["adm_in_channels"], generator=g)
    concat = concat_entry(g)
    out = {"cfg": cfg, "shapes": shapes, "x": x, "context": ctx, "y": y, "concat": concat, "seed": SEED, "cases": {}}
    for tag, kw in CONCAT_CASES:
        if kw["objective_type"] == "rf":
            sig = torch.tensor([0.6, 0.3])
            denoiser, weighting = nd.Denoiser(preconditioning=nd.RectifiedFlowXLPreconditioning()), nd.RectifiedFlowWeighting()
        else:
            sig = torch.tensor([0.8, 4.2])
            denoiser = nd.DiscreteDenoiser(preconditioning=nd.EpsPreconditioning(), num_idx=1000, discretization=nd.LegacyDDPMDiscretization())
            weighting = nd.EpsWeighting()
        loss_fn = StandardDiffusionLoss(sigma_generator=FixedSigma(sig), loss_weighting=weighting, **kw)
        for p_ in net.parameters():
            p_.grad = None
        # the draws _forward makes, in its order, recorded so that the HIP path can be fed the same ones
        torch.manual_seed(SEED)
        _t = torch.rand((B,), dtype=torch.float64)
        noise = torch.randn_like(x)
        torch.manual_seed(SEED)
        loss, extra = loss_fn._forward(wrapper, denoiser, {"crossattn": ctx, "vector": y, "concat": concat}, x, {}, return_dict=True)
        loss.mean().backward()
        assert torch.equal(extra["t"], _t)
        grads = {k: grad_rows(p_.grad.detach().clone()) for k, p_ in net.named_parameters() if k in GRAD_KEYS}
        assert grads["input_blocks.0.0.weight"].shape[1] == 9
        gnorm = {k: float(p_.grad.norm()) for k, p_ in net.named_parameters()}
        out["cases"][tag] = dict(kwargs=kw, sigma=sig, noise=noise, loss=loss.detach(), grads=grads, grad_norms=gnorm, weighting=type(weighting).__name__)
        w0 = grads["input_blocks.0.0.weight"]
        print(f"concat {tag}: loss={loss.tolist()} |d conv_in| latent columns {float(w0[:, :4].norm()):.4f} concat columns {float(w0[:, 4:].norm()):.4f}")

    # sampling: one guided denoiser evaluation, the two halves with their own concat tensors
    denoiser = nd.DiscreteDenoiser(preconditioning=nd.EpsPreconditioning(), num_idx=1000, discretization=nd.LegacyDDPMDiscretization())
    guider = VanillaCFG(CFG_SCALE)
    sigma = torch.tensor([2.5, 0.9])
    xs = x + sigma[:, None, None, None] * torch.randn(CONCAT_SHAPE, generator=g)
    cond = {"crossattn": ctx, "vector": y, "concat": concat}
    uc = {"crossattn": torch.randn(B, 7, cfg["context_dim"], generator=g), "vector": torch.zeros(B, cfg["adm_in_channels"]), "concat": concat_entry(g)}
    assert not torch.equal(uc["concat"], cond["concat"])
    with torch.no_grad():
        denoised = guider(denoiser(wrapper, *guider.prepare_inputs(xs, sigma, cond, uc), "D"), sigma)
        swapped = guider(denoiser(wrapper, *guider.prepare_inputs(xs, sigma, dict(cond, concat=uc["concat"]), dict(uc, concat=cond["concat"])), "D"), sigma)
    # (how far apart the two assignments of the concat tensors are: a test tolerance must be well below this to notice a swap)
    swap_distance = float((swapped - denoised).abs().max() / denoised.abs().max())
    out["sample"] = dict(x=xs, sigma=sigma, scale=CFG_SCALE, cond=cond, uc=uc, denoised=denoised, swap_distance=swap_distance)
    print(f"concat sample: |D|={float(denoised.abs().mean()):.5f} distance of the swapped assignment {swap_distance:.4f}")
    save_fixture(out, "concat_tiny")


if __name__ == "__main__":
    nd, _ = import_reference()
    concat_case(nd)
