"""Golden fixtures for the ADM block family (guided-diffusion ResBlocks): scale-shift norm, the up / down ResBlock, the parameter-free
Upsample / Downsample, and a tiny UNetModel built from them.  Run from the repository root on a machine that has the reference checkout:

    python -m tests.golden.make_golden_adm

Writes adm_blocks.{safetensors,json} and unet_adm_tiny.{safetensors,json} (data only: inputs are rebuilt by the tests from the case name).
The reference runs in fp32 on bf16-exact inputs.  To keep the files small an activation larger than PIXEL_SAMPLE_MIN elements is stored at
PIXEL_SAMPLES pixel positions (all images, all channels; the positions are in the fixture) plus its norm, and a weight gradient as its
first BLOCK_SAMPLE_ROWS rows (of a convolution kernel: the first CONV_SAMPLE_CIN input channels of those rows) plus its norm."""
from __future__ import annotations

import zlib

import torch

from tests.golden.fixture_io import save_fixture
from tests.golden.make_golden import BLOCK_SAMPLE_ROWS, block_inputs, block_upstream, import_reference, synth_state_dict

ADM_BLOCK_CASES = {
    # name: (constructor kwargs, input shapes)
    "ssn_320_640": (dict(channels=320, emb_channels=1280, dropout=0.0, out_channels=640, use_scale_shift_norm=True), dict(x=(2, 320, 16, 16), emb=(2, 1280))),
    "down_320": (dict(channels=320, emb_channels=1280, dropout=0.0, out_channels=320, down=True), dict(x=(2, 320, 14, 10), emb=(2, 1280))),
    "down_ssn_odd": (dict(channels=64, emb_channels=256, dropout=0.0, out_channels=96, down=True, use_scale_shift_norm=True), dict(x=(2, 64, 7, 10), emb=(2, 256))),
    "up_ssn_640": (dict(channels=640, emb_channels=1280, dropout=0.0, out_channels=640, up=True, use_scale_shift_norm=True), dict(x=(1, 640, 8, 8), emb=(1, 1280))),
    "up_skipconv": (dict(channels=64, emb_channels=256, dropout=0.0, out_channels=96, up=True, use_conv=True), dict(x=(2, 64, 5, 6), emb=(2, 256))),
}
PIXEL_SAMPLE_MIN = 16384
PIXEL_SAMPLES = 16
CONV_SAMPLE_CIN = 64

UNET_ADM_TINY = dict(
    in_channels=4, model_channels=32, out_channels=4, channel_mult=[1, 2, 2], num_res_blocks=1, attention_resolutions=[2], num_head_channels=16,
    transformer_depth=1, context_dim=64, use_linear_in_transformer=True, num_classes="sequential", adm_in_channels=48,
    use_scale_shift_norm=True, resblock_updown=True, spatial_transformer_attn_type="torch-sdp", use_checkpoint=False,
)
UNET_ADM_PLAIN_RESAMPLE = dict(UNET_ADM_TINY, use_scale_shift_norm=False, resblock_updown=False, conv_resample=False)
UNET_ADM_SHAPE = (2, 4, 16, 24)
UNET_ADM_GRAD_KEYS = [
    "input_blocks.0.0.weight", "input_blocks.1.0.emb_layers.1.weight", "input_blocks.1.0.out_layers.0.weight", "input_blocks.2.0.in_layers.2.weight",
    "input_blocks.2.0.emb_layers.1.weight", "input_blocks.2.0.out_layers.0.bias", "input_blocks.3.0.skip_connection.weight",
    "input_blocks.3.1.transformer_blocks.0.attn2.to_k.weight", "middle_block.0.emb_layers.1.bias", "middle_block.2.out_layers.3.weight",
    "output_blocks.1.1.in_layers.0.weight", "output_blocks.1.1.out_layers.3.weight", "output_blocks.3.2.emb_layers.1.weight", "output_blocks.4.0.in_layers.2.weight",
    "time_embed.0.weight", "label_emb.0.2.bias", "out.2.weight",
]


def sample_pixels(name: str, H: int, W: int) -> list:
    """the pixel positions (h * W + w) at which a large activation is stored: the four corners and seeded others"""
    if H * W <= PIXEL_SAMPLES:
        return list(range(H * W))
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/pixels/{H}x{W}".encode()) & 0x7FFFFFFF)
    picked = [0, W - 1, (H - 1) * W, H * W - 1]
    for p in torch.randperm(H * W, generator=g).tolist():
        if len(picked) == PIXEL_SAMPLES:
            break
        if p not in picked:
            picked.append(p)
    return sorted(picked)


def sampled(name: str, t: torch.Tensor) -> dict:
    """an [N, C, H, W] activation as stored: whole when small, else the sampled pixels [N, C, P]; always with its norm"""
    t = t.detach()
    if t.dim() != 4 or t.numel() <= PIXEL_SAMPLE_MIN:
        return dict(full=t.contiguous(), norm=float(t.norm()))
    pix = sample_pixels(name, t.shape[2], t.shape[3])
    return dict(pixels=pix, values=t.flatten(2)[:, :, pix].contiguous(), norm=float(t.norm()), shape=list(t.shape))


def grad_rows(g: torch.Tensor) -> torch.Tensor:
    if g.dim() == 4:
        return g[:BLOCK_SAMPLE_ROWS, :CONV_SAMPLE_CIN].contiguous()
    return (g[:BLOCK_SAMPLE_ROWS] if g.dim() >= 2 else g).contiguous()


def blocks_case():
    from neurosis.modules.diffusion.openaimodel import ResBlock

    fixture = {}
    for name, (kw, in_shapes) in ADM_BLOCK_CASES.items():
        blk = ResBlock(**kw).eval()
        shapes = {k: list(v.shape) for k, v in blk.state_dict().items()}
        blk.load_state_dict(synth_state_dict(shapes))
        ins = {k: v.clone().requires_grad_(True) for k, v in block_inputs(name, in_shapes).items()}
        out = blk(ins["x"], ins["emb"])
        out.backward(block_upstream(name, out.shape))
        case = dict(shapes=shapes, params=[k for k, _ in blk.named_parameters()], out_shape=list(out.shape), out=sampled(f"{name}/out", out),
                    d_x=sampled(f"{name}/d_x", ins["x"].grad), d_emb=ins["emb"].grad.detach().clone(),
                    grad_norms={k: float(p.grad.norm()) for k, p in blk.named_parameters()},
                    g={k: grad_rows(p.grad.detach()) for k, p in blk.named_parameters()})
        fixture[name] = case
        print(f"adm block {name}: out {tuple(out.shape)} |out| {float(out.abs().mean()):.4f} params {sum(p.numel() for p in blk.parameters())}")
    save_fixture(fixture, "adm_blocks")


def unet_inputs():
    N, Cc, H, W = UNET_ADM_SHAPE
    ins = block_inputs("unet_adm_tiny", dict(x=(N, Cc, H, W), context=(N, 7, UNET_ADM_TINY["context_dim"]), y=(N, UNET_ADM_TINY["adm_in_channels"])))
    ins["timesteps"] = torch.tensor([37, 811][:N])
    return ins


def zero_gradient_noise(net, ins, grad_norms: dict) -> dict:
    """A convolution bias in front of a one-channel-per-group GroupNorm has an analytically zero gradient (fp32: ~1e-5 here).  A bf16 path
    sums the bf16-rounded gradient of the convolution's output instead, which leaves rounding noise in proportion to that gradient.  This
    is that noise for the reference's own fp32 gradient: key -> |sum over n, h, w of bf16(d out)|, for every such bias.  Without scale-shift
    the emb projection adds into the same convolution output, so its gradients are zero in the same way: their noise is the per-image
    sum e[n, c] = sum over h, w of bf16(d out) folded like the Linear's backward (bias: sum over n; weight: e^T @ input)."""
    gmax = max(grad_norms.values())
    keys = [k for k, n in grad_norms.items() if n <= 1e-6 * gmax]
    noise, hooks, mods, lin_in = {}, [], dict(net.named_modules()), {}
    for k in keys:
        owner, leaf = k.rsplit(".", 1)
        if owner.endswith("emb_layers.1"):
            conv = owner[: -len("emb_layers.1")] + "in_layers.2"
            assert grad_norms[conv + ".bias"] <= 1e-6 * gmax, k

            def hook(m, gin, gout, k=k, owner=owner, leaf=leaf):
                e = gout[0].bfloat16().float().sum((2, 3))
                noise[k] = float(e.sum(0).norm() if leaf == "bias" else (e.t() @ lin_in[owner]).norm())
            hooks.append(mods[owner].register_forward_hook(lambda m, a, o, owner=owner: lin_in.__setitem__(owner, a[0].detach())))
            hooks.append(mods[conv].register_full_backward_hook(hook))
        else:
            assert leaf == "bias", k

            def hook(m, gin, gout, k=k):
                noise[k] = float(gout[0].bfloat16().float().sum((0, 2, 3)).norm())
            hooks.append(mods[owner].register_full_backward_hook(hook))
    out = net(ins["x"], ins["timesteps"], ins["context"], ins["y"])
    out.backward(block_upstream("unet_adm_tiny", out.shape))
    for h in hooks:
        h.remove()
    net.zero_grad()
    assert sorted(noise) == sorted(keys)
    return noise


def unet_case(nd):
    ins = unet_inputs()
    fixture = {}
    for name, cfg in (("updown_ssn", UNET_ADM_TINY), ("plain_resample", UNET_ADM_PLAIN_RESAMPLE)):
        net = nd.UNetModel(**cfg).eval()
        shapes = {k: list(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict(synth_state_dict(shapes))
        case = dict(cfg=cfg, shapes=shapes)
        out = net(ins["x"], ins["timesteps"], ins["context"], ins["y"])
        out.backward(block_upstream("unet_adm_tiny", out.shape))
        # (the parameter-free Downsample of the second case has no input_blocks.2.0.* parameters)
        case["grads"] = {k: p.grad.detach().clone() for k, p in net.named_parameters() if k in UNET_ADM_GRAD_KEYS}
        assert name != "updown_ssn" or len(case["grads"]) == len(UNET_ADM_GRAD_KEYS), set(UNET_ADM_GRAD_KEYS) - set(case["grads"])
        case["grad_norms"] = {k: float(p.grad.norm()) for k, p in net.named_parameters()}
        case["bf16_zero_grad_noise"] = zero_gradient_noise(net, ins, case["grad_norms"])
        case["F_out"] = out.detach().clone()
        fixture[name] = case
        print(f"adm unet {name}: |out| {float(out.abs().mean()):.4f} params {sum(p.numel() for p in net.parameters())}")
    save_fixture(fixture, "unet_adm_tiny")


if __name__ == "__main__":
    torch.manual_seed(0)
    nd, _ = import_reference()
    blocks_case()
    unet_case(nd)
