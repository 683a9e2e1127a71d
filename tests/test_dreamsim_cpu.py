"""DreamSim without a GPU: class paths, constructor signatures, state-dict keys and shapes against the fixture the reference produced
(tests/golden/make_golden_dreamsim.py), the from_pretrained round trip, the refusals, the interpolated position table, and the new entry
points in the header, the binding and the exports.  The arithmetic on the GPU is tests/test_dreamsim_gpu.py."""
import inspect
import logging
import math
import re
from functools import lru_cache
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from neurosis_amd import lib, ops
from neurosis_amd.modules.autoencoding import losses as L
from neurosis_amd.modules.losses import dreamsim as D
from neurosis_amd.modules.losses.dreamsim import vit as V
from tests import dreamsim_reference as R
from tests.dreamsim_fixture import checked_state
from tests.golden.fixture_io import load_fixture

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("nk_vit_add_ln", "nk_vit_cls_head_fwd", "nk_vit_cls_head_bwd", "nk_vit_patchify", "nk_vit_patchify_bwd", "nk_vit_tokens", "nk_vit_tokens_bwd", "nk_dreamsim_head_fwd", "nk_dreamsim_head_bwd")


@lru_cache(maxsize=None)
def fixture():
    return load_fixture("dreamsim_tiny")


def tiny_ensemble(**kw):
    fx = fixture()
    return D.DreamsimEnsemble(num_classes=tuple(fx["num_classes"]), vit_config=fx["vit_config"], **kw)


def test_class_paths_resolve_under_the_prefix_swap():
    from tests.test_config_classpaths import resolve, swap

    assert resolve(swap("neurosis.modules.autoencoding.losses.AutoencoderDreamsim")) is L.AutoencoderDreamsim
    assert "AutoencoderDreamsim" in L.__all__
    assert resolve(swap("neurosis.modules.losses.dreamsim.model.DreamsimEnsemble")) is D.DreamsimEnsemble
    assert resolve(swap("neurosis.modules.losses.dreamsim.model.DreamsimModel")) is D.DreamsimModel
    assert resolve(swap("neurosis.modules.losses.dreamsim.vit.VisionTransformer")) is D.VisionTransformer
    assert resolve(swap("neurosis.modules.losses.dreamsim.common.get_act_layer")) is D.get_act_layer


def test_constructor_signatures_are_the_references():
    fx = fixture()
    got = {k: p for k, p in inspect.signature(D.VisionTransformer.__init__).parameters.items() if k not in ("self", "kwargs")}
    assert list(got) == list(fx["vit_args"])
    for k, default in fx["vit_args"].items():
        if default is not None:
            assert got[k].default == default, k
    assert [k for k in inspect.signature(D.vit_base_dreamsim).parameters if k != "kwargs"] == fx["vit_base_args"]

    def defaults(fn):
        return {k: (p.default, p.kind) for k, p in inspect.signature(fn).parameters.items() if k != "self"}

    ens = defaults(D.DreamsimEnsemble.__init__)
    assert list(ens) == ["image_size", "patch_size", "layer_norm_eps", "num_classes", "do_resize", "vit_config"]
    assert ens["layer_norm_eps"][0] == (1e-6, 1e-5, 1e-5) and ens["num_classes"][0] == (0, 512, 512) and ens["image_size"][0] == 224
    assert ens["vit_config"] == (None, inspect.Parameter.KEYWORD_ONLY)
    one = defaults(D.DreamsimModel.__init__)
    assert list(one) == ["image_size", "patch_size", "layer_norm_eps", "pre_norm", "act_layer", "img_mean", "img_std", "do_resize", "vit_config"]
    assert one["vit_config"] == (None, inspect.Parameter.KEYWORD_ONLY) and one["act_layer"][0] == "gelu" and one["pre_norm"][0] is False
    loss = defaults(L.AutoencoderDreamsim.__init__)
    want = dict(dreamsim_name_or_path="neggles/dreamsim:ensemble_vitb16", dreamsim_weight=1.0, dreamsim_ensemble=True, recon_type="l1", recon_weight=1.0,
                resize_input=False, resize_target=False, extra_log_keys=[], rescale_input=True, delay_setup=False, dreamsim_compile=False, vit_config=None)
    assert list(loss) == list(want) and {k: v[0] for k, v in loss.items()} == want
    assert loss["vit_config"][1] == inspect.Parameter.KEYWORD_ONLY


def test_state_dict_keys_and_shapes_match_the_references():
    fx = fixture()
    clip = D.vit_base_dreamsim(num_classes=512, pre_norm=True, act_layer="quick_gelu")
    assert {k: list(v.shape) for k, v in clip.state_dict().items()} == fx["vit_b_clip_keys"]
    assert list(clip.state_dict()) == list(fx["vit_b_clip_keys"])
    dino = D.vit_base_dreamsim(num_classes=0)
    assert {k: list(v.shape) for k, v in dino.state_dict().items()} == fx["vit_b_dino_keys"]
    assert not any(p.requires_grad for p in clip.parameters()) and not clip.training
    assert clip.train().training is False                                  # frozen: there is no train mode
    ens = tiny_ensemble()
    assert {k: list(v.shape) for k, v in ens.state_dict().items()} == fx["state_shapes"]
    ens.load_state_dict(checked_state(fx), strict=True)


def test_from_pretrained_round_trip_and_hub_refusal(tmp_path):
    fx = fixture()
    ens = tiny_ensemble(do_resize=True, image_size=32)
    ens.load_state_dict(checked_state(fx))
    ens.save_pretrained(tmp_path / "ens")
    assert sorted(p.name for p in (tmp_path / "ens").iterdir()) == ["config.json", "diffusion_pytorch_model.safetensors"]
    back = D.DreamsimEnsemble.from_pretrained(tmp_path / "ens", local_files_only=True, vit_config=fx["vit_config"])
    assert back.do_resize and back.image_size == (32, 32) and back.config == ens.config
    assert all(torch.equal(a, b) for a, b in zip(ens.state_dict().values(), back.state_dict().values()))
    assert not back.training and not any(p.requires_grad for p in back.parameters())
    one = D.DreamsimModel(pre_norm=True, act_layer="quick_gelu", layer_norm_eps=1e-5, vit_config={**fx["vit_config"], "num_classes": 16})
    one.save_pretrained(tmp_path / "one")
    again = D.DreamsimModel.from_pretrained(tmp_path / "one", vit_config={**fx["vit_config"], "num_classes": 16})
    assert again.pre_norm and again.extractor.quick_gelu and again.extractor.head.weight.shape == (16, 128)
    with pytest.raises(ValueError, match="other DreamSim class"):
        D.DreamsimEnsemble.from_pretrained(tmp_path / "one", vit_config=fx["vit_config"])
    with pytest.raises(FileNotFoundError, match="no hub access"):
        D.DreamsimEnsemble.from_pretrained("neggles/dreamsim")
    # the loss class: the reference's default names the hub
    with pytest.raises(FileNotFoundError, match="no hub access"):
        L.AutoencoderDreamsim()
    loss = L.AutoencoderDreamsim(dreamsim_name_or_path=str(tmp_path / "ens"), vit_config=fx["vit_config"])
    assert isinstance(loss.dreamsim_loss, D.DreamsimEnsemble) and any(k.startswith("dreamsim_loss.dino.") for k in loss.state_dict())


def test_autoencoder_dreamsim_configures_like_autoencoder_perceptual(caplog):
    fx = fixture()
    with caplog.at_level(logging.INFO, logger=L.__name__):
        loss = L.AutoencoderDreamsim(delay_setup=True, dreamsim_compile=True, dreamsim_weight=0.7, recon_type="mse", resize_target=True, vit_config=fx["vit_config"])
    assert loss.dreamsim_loss is None and list(loss.state_dict()) == [] and loss.forward_keys == ["split"]
    assert any("dreamsim_compile" in r.getMessage() and "ignored" in r.getMessage() for r in caplog.records)
    loss.configure_model()
    first = loss.dreamsim_loss
    assert isinstance(first, D.DreamsimEnsemble)
    loss.configure_model()
    assert loss.dreamsim_loss is first and list(loss.get_trainable_parameters()) == []
    cfg = loss.engine_settings()
    assert cfg["perceptual_only"] and cfg["perceptual_kind"] == "dreamsim" and cfg["discriminator"] is None and cfg["resize"] == "target"
    assert cfg["rec_loss_type"] == "l2" and cfg["perceptual_weight"] == 0.7
    assert isinstance(L.AutoencoderDreamsim(dreamsim_ensemble=False, vit_config=fx["vit_config"]).dreamsim_loss, D.DreamsimModel)
    with pytest.raises(RuntimeError, match="AutoencodingEngine"):
        loss(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), split="train")
    with pytest.raises(ValueError, match="resize_input and resize_target"):
        L.AutoencoderDreamsim(resize_input=True, resize_target=True, delay_setup=True)
    with pytest.raises(ValueError):
        L.AutoencoderDreamsim(recon_type="huber", delay_setup=True)


def test_engine_takes_the_dreamsim_loss():
    from neurosis_amd.models.autoencoder import AutoencodingEngine
    from neurosis_amd.modules.diffusion.model import Decoder, Encoder

    cfg = load_fixture("vae_train_tiny")["cfg"]
    loss = L.AutoencoderDreamsim(delay_setup=True, dreamsim_weight=0.5, vit_config=fixture()["vit_config"])
    eng = AutoencodingEngine(encoder=Encoder(**cfg), decoder=Decoder(**cfg), loss=loss)
    assert eng.perceptual_only and eng.perceptual_kind == "dreamsim" and eng.perceptual_weight == 0.5 and eng.discriminator is None
    eng.loss.configure_model()
    assert any(k.startswith("loss.dreamsim_loss.clip2.") for k in eng.state_dict())
    # vit_config's num_classes is the head width of the ensemble's towers that have a head
    ens = L.AutoencoderDreamsim(vit_config={**fixture()["vit_config"], "num_classes": 16}).dreamsim_loss
    assert {k: list(v.shape) for k, v in ens.state_dict().items()} == fixture()["state_shapes"] and ens.config["num_classes"] == [0, 16, 16]
    assert AutoencodingEngine(encoder=Encoder(**cfg), decoder=Decoder(**cfg), loss="l2").perceptual_kind == "lpips"


def test_refusals_name_what_is_not_built():
    with pytest.raises(NotImplementedError, match="dynamic_pad"):
        D.VisionTransformer(dynamic_pad=True)
    with pytest.raises(NotImplementedError, match="get_intermediate_layers"):
        D.vit_base_dreamsim(embed_dim=128, depth=1, num_heads=2).get_intermediate_layers(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="not supported"):
        D.get_act_layer("relu")
    with pytest.raises(NotImplementedError, match="head dim"):
        D.VisionTransformer(embed_dim=96, num_heads=2, depth=1)
    assert D.get_act_layer("gelu") is torch.nn.GELU and D.get_act_layer("quick_gelu") is D.QuickGELU
    t = D.vit_base_dreamsim(embed_dim=128, depth=1, num_heads=2, drop_rate=0.1, attn_drop_rate=0.2, drop_path_rate=0.3)      # accepted, inert
    assert not t.training
    with pytest.raises(NotImplementedError, match="CPU"):
        tiny_ensemble()(torch.zeros(2, 1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="CPU"):
        ops.dreamsim_head(torch.zeros(2, 1, 8))
    with pytest.raises(NotImplementedError, match="CPU"):
        ops.vit_patchify(torch.zeros(1, 3, 32, 32), 16, ops.vit_affine((1, 1, 1), (0, 0, 0)))


def test_position_table_matches_the_fixture_and_f_interpolate():
    fx = fixture()
    ens = tiny_ensemble()
    ens.load_state_dict(checked_state(fx))
    for name in ("dino", "clip1", "clip2"):
        tower = getattr(ens, name)
        native = tower.interpolate_pos_encoding(32, 32)
        assert torch.equal(native, tower.pos_embed[0]) and torch.equal(native, fx["cases"]["32"]["pos"][name])
        got, want = tower.interpolate_pos_encoding(48, 48), fx["cases"]["48"]["pos"][name]              # 2 x 2 -> 3 x 3
        assert got.shape == want.shape == (10, 128)
        assert float((got - want).abs().max()) <= 2e-6 * float(want.abs().max())
    # ViT-B's 14 x 14 -> 16 x 16 (a 256 x 256 image) against F.interpolate with the scale factor PASSED, as the reference calls it
    torch.manual_seed(5)
    vit_b = D.vit_base_dreamsim(num_classes=0)
    vit_b.pos_embed.data.normal_(std=0.02)
    got = vit_b.interpolate_pos_encoding(256, 256)
    grid = vit_b.pos_embed[:, 1:].reshape(1, 14, 14, 768).permute(0, 3, 1, 2)
    sf = 16.1 / 14.0
    want = F.interpolate(grid, scale_factor=(sf, sf), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).reshape(256, 768)
    assert got.shape == (257, 768) and torch.equal(got[0], vit_b.pos_embed[0, 0])
    assert float((got[1:] - want).abs().max()) <= 2e-6 * float(want.abs().max())
    # the out / in ratio (what F.interpolate uses when only a size is given) is another table: the 0.1 matters
    other = F.interpolate(grid, size=(16, 16), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).reshape(256, 768)
    assert float((got[1:] - other).abs().max()) > 1e-4 * float(want.abs().max())
    M = V.bicubic_axis_matrix(14, 16, sf)
    assert M.shape == (16, 14) and abs(M.sum(axis=1) - 1.0).max() < 1e-12
    for hw in ((32, 48), (48, 32), (16, 64)):
        with pytest.raises(ValueError, match="positional encoding"):
            ens.dino.interpolate_pos_encoding(*hw)


def test_position_table_is_cached_per_size():
    ens = tiny_ensemble()
    a = ens.dino.pos_table(48, 48)
    assert ens.dino.pos_table(48, 48) is a
    with torch.no_grad():
        ens.dino.pos_embed.add_(1.0)
    assert ens.dino.pos_table(48, 48) is not a                             # a new value of the parameter is a new table
    # a size seen for the first time while a launch sequence is being recorded raises instead of copying from the host
    with ops.capture_scope():
        assert ens.dino.pos_table(48, 48) is ens.dino.pos_table(48, 48)
        with pytest.raises(RuntimeError, match="before capturing"):
            ens.dino.pos_table(64, 64)


def test_restatement_used_by_the_gpu_tests_reproduces_the_fixture():
    """tests/dreamsim_reference.py (the yardstick of the engine-step test) against what the reference's own classes recorded"""
    fx = fixture()
    sd = {k: v.double() for k, v in checked_state(fx).items()}
    for size, case in fx["cases"].items():
        r = case["recons"].double().requires_grad_(True)
        emb, d = R.ensemble(sd, case["inputs"].double().clamp(-1, 1), r.clamp(-1, 1), fx["vit_config"]["num_heads"])
        (grad,) = torch.autograd.grad(d.sum(), r)
        for name in emb:
            assert float((emb[name].detach() - case["emb"][name]).abs().max()) <= 1e-5 * float(case["emb"][name].abs().max()), (size, name)
        assert float((d.detach() - case["d"]).abs().max()) <= 1e-5 and float((grad - case["grad"]).abs().max()) <= 1e-5 * float(case["grad"].abs().max())
        assert float(case["d"].min()) >= 0.05


def test_new_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "neurosis_hip.h").read_text(), flags=re.S)
    l = lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in lib.SIGNATURES and hasattr(l, name), name
    assert l.nk_abi_version() == 5
    for fn in ("vit_add_ln", "vit_cls_head", "vit_patchify", "vit_patchify_bwd", "vit_tokens", "vit_tokens_bwd", "dreamsim_head"):
        assert callable(getattr(ops, fn))
    assert "vit.hip" in (ROOT / "neurosis_amd" / "csrc" / "Makefile").read_text()


def test_head_dim_is_what_the_attention_kernels_take():
    assert V.HEAD_DIM == 64 and 768 // 12 == V.HEAD_DIM and math.isclose(64 ** -0.5, 0.125)
