"""Concat-conditioned UNets (inpainting / edit / upscale models), the parts that need no GPU: the two _cat entry points are declared and
bound, their torch ops are registered without a CPU kernel, IdentityEncoder files a 4-D batch entry under "concat" through
GeneralConditioner and resolves from the reference's class path, and OpenAIWrapper.fused_unet draws the boundary of the fused route."""
import importlib
import re
from pathlib import Path

import pytest
import torch

from neurosis_amd import lib

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = {"nk_edm_prepare_cat": "nk_edm_prepare", "nk_sample_prepare_cat": "nk_sample_prepare"}


def _header_args(name: str) -> list:
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "neurosis_hip.h").read_text(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/neurosis_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NEW_SYMBOLS))
def test_entry_points_are_declared_and_bound(name):
    args = _header_args(name)
    assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == len(args)
    # the old entry point extended by the concat tensor(s) and Ce, nothing else
    old = _header_args(NEW_SYMBOLS[name])
    added = [a.split()[-1].lstrip("*") for a in args if a not in old]
    assert added == (["extra", "Ce"] if name == "nk_edm_prepare_cat" else ["extra_u", "extra_c", "Ce"])
    assert hasattr(lib.load(), name)


def test_ops_are_registered_and_have_no_cpu_kernel():
    import neurosis_amd.torch_ops as T

    o = torch.ops.neurosis_hip
    assert "edm_prepare_cat" in T.OPS and "sample_prepare_cat" in T.OPS
    f32 = torch.float32
    m = lambda *s: torch.empty(*s, dtype=f32, device="meta")
    zt, net_in = o.edm_prepare_cat(m(2, 4, 16, 24), m(2, 4, 16, 24), m(2), m(2), m(2, 5, 16, 24), 16)
    assert zt.shape == (2, 4, 16, 24) and net_in.shape == (2 * 16 * 24, 16) and net_in.dtype == torch.bfloat16
    assert o.sample_prepare_cat(m(2, 4, 16, 24), m(2), m(2, 5, 16, 24), m(2, 5, 16, 24), 16, 2).shape == (2 * 2 * 16 * 24, 16)
    assert o.sample_prepare_cat(m(2, 4, 16, 24), m(2), None, m(2, 5, 16, 24), 16, 1).shape == (2 * 16 * 24, 16)
    z = lambda *s: torch.zeros(*s, dtype=f32)
    with pytest.raises(NotImplementedError, match="CPU"):
        o.edm_prepare_cat(z(1, 4, 2, 2), z(1, 4, 2, 2), z(1), z(1), z(1, 1, 2, 2), 8)
    with pytest.raises(NotImplementedError, match="CPU"):
        o.sample_prepare_cat(z(1, 4, 2, 2), z(1), None, z(1, 1, 2, 2), 8, 1)


def test_identity_encoder_in_a_general_conditioner():
    from neurosis_amd.modules.encoders import GeneralConditioner, IdentityEncoder, PrecomputedEmbedder

    g = torch.Generator().manual_seed(3)
    mask, masked, ctx = torch.rand(3, 1, 4, 6, generator=g), torch.randn(3, 4, 4, 6, generator=g), torch.randn(3, 7, 8, generator=g)
    batch = {"mask": mask, "masked": masked, "ctx": ctx}
    enc = IdentityEncoder(input_key="mask")
    assert enc(mask) is mask and enc.encode(mask) is mask and not list(enc.parameters())
    cond = GeneralConditioner([enc, PrecomputedEmbedder(input_key="ctx")])(batch)
    assert set(cond) == {"concat", "crossattn"} and torch.equal(cond["concat"], mask)
    # two of them: joined on the channel axis in embedder order
    both = GeneralConditioner([IdentityEncoder(input_key="mask"), IdentityEncoder(input_key="masked")])
    assert torch.equal(both(batch)["concat"], torch.cat((mask, masked), 1))
    swapped = GeneralConditioner([IdentityEncoder(input_key="masked"), IdentityEncoder(input_key="mask")])
    assert torch.equal(swapped(batch)["concat"], torch.cat((masked, mask), 1))
    out = both(batch, force_zero_embeddings=["masked"])["concat"]
    assert torch.equal(out[:, :1], mask) and float(out[:, 1:].abs().max()) == 0.0
    dropped = GeneralConditioner([IdentityEncoder(input_key="mask", ucg_rate=1.0), IdentityEncoder(input_key="masked")])(batch)["concat"]
    assert float(dropped[:, :1].abs().max()) == 0.0 and torch.equal(dropped[:, 1:], masked)


def test_identity_encoder_resolves_from_the_reference_class_path():
    from tests.test_config_classpaths import resolve, swap

    cls = resolve(swap("neurosis.modules.encoders.misc.IdentityEncoder"))
    assert cls is importlib.import_module("neurosis_amd.modules.encoders").IdentityEncoder
    assert cls(input_key="mask", ucg_rate=0.1).input_key == "mask"


class _OnDevice(torch.Tensor):
    """a meta tensor that says it lives on the GPU: fused_unet only looks at shapes, devices and flags"""
    is_cuda = property(lambda self: True)


def _dev(*shape, requires_grad=False):
    return torch.empty(*shape, device="meta", requires_grad=requires_grad).as_subclass(_OnDevice)


def test_fused_unet_boundary_for_concat_conditioning():
    import neurosis_amd.modules.diffusion as D
    from tests.golden.make_golden import UNET_TINY

    with torch.device("meta"):
        net9, net4 = D.UNetModel(**dict(UNET_TINY, in_channels=9)), D.UNetModel(**UNET_TINY)
    w9, w4 = D.OpenAIWrapper(net9), D.OpenAIWrapper(net4)
    x = _dev(2, 4, 16, 24)
    assert w9.fused_unet(x, {"concat": _dev(2, 5, 16, 24)}, {}) is net9
    assert w4.fused_unet(x, {}, {}) is net4
    assert w4.fused_unet(x, {"concat": _dev(0)}, {}) is net4                       # an empty tensor means no concat, as in forward
    assert w4.fused_unet(torch.empty(2, 4, 16, 24, device="meta"), {}, {}) is None    # (latents not on the GPU)
    with pytest.raises(ValueError, match=r"4 latent \+ 4 concat.*in_channels = 9"):
        w9.fused_unet(x, {"concat": _dev(2, 4, 16, 24)}, {})
    with pytest.raises(ValueError, match=r"4 latent \+ 5 concat.*in_channels = 4"):
        w4.fused_unet(x, {"concat": _dev(2, 5, 16, 24)}, {})
    # what still takes the generic route
    assert w9.fused_unet(x, {"concat": _dev(2, 5, 3, 16, 24)}, {}) is None           # video
    assert w9.fused_unet(x, {"concat": _dev(2, 5, 16, 24, requires_grad=True)}, {}) is None
    assert w9.fused_unet(x, {"concat": _dev(2, 5, 16, 24)}, {"num_video_frames": 3}) is None
    assert w9.fused_unet(x, {"concat": _dev(2, 5, 16, 12)}, {}) is None              # not the latents' H, W
    assert w9.fused_unet(x, {"concat": torch.empty(2, 5, 16, 24)}, {}) is None       # on another device
