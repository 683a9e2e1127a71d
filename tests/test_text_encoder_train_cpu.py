"""Host side of the trainable text towers (configs/sdxl/sdxl-te.example.yaml): the learning-rate scheduler that config names against the
reference's own, which parameters each embedder trains, the settings a trainable embedder refuses, and the engine's refusal of trainable
embedders (the UNet's gradient of its conditioning is not built yet).  No GPU: the towers are built on the CPU or the meta device."""
import json
import math
from pathlib import Path

import pytest
import torch

G = Path(__file__).resolve().parent / "golden"

# the two embedders and the scheduler as configs/sdxl/sdxl-te.example.yaml gives them (conditioner.emb_models[0:2], scheduler)
SDXL_TE_CLIP_L = dict(layer="hidden", layer_idx=11, input_key="caption", is_trainable=True, base_lr=1.0)
SDXL_TE_BIGG = dict(arch="ViT-bigG-14", version=None, freeze=True, layer="penultimate", always_return_pooled=True, legacy=False, input_key="caption",
                    is_trainable=True, base_lr=1.0)
SDXL_TE_SCHEDULER = dict(first_cycle_steps=50, cycle_mult=1.0, min_lr=3e-7, warm_up_steps=25, gamma=0.9)


def _groups(initial_lrs):
    return [{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr, "initial_lr": lr} for lr in initial_lrs]


@pytest.mark.parametrize("case", json.loads((G / "lr_legacy_cosine.json").read_text())["cases"], ids=lambda c: c["name"])
def test_legacy_cosine_scheduler_matches_reference(case):
    """the learning rate of every group after every step, as the reference's LegacyCosineAnnealingWarmupRestarts sets it
    (tests/golden/make_golden_scheduler.py)"""
    from neurosis_amd.schedulers import LegacyCosineAnnealingWarmupRestarts

    opt = torch.optim.SGD(_groups(case["initial_lrs"]), lr=1.0)
    sched = LegacyCosineAnnealingWarmupRestarts(opt, **case["kwargs"])
    got = [[g["lr"] for g in opt.param_groups]]
    for e in case["epochs"] if case["epochs"] is not None else [None] * case["steps"]:
        sched.step() if e is None else sched.step(e)
        got.append([float(g["lr"]) for g in opt.param_groups])
    assert len(got) == len(case["lrs"])
    for i, (a, b) in enumerate(zip(got, case["lrs"])):
        for x, y in zip(a, b):
            assert math.isclose(x, y, rel_tol=1e-12, abs_tol=1e-300), (case["name"], i, a, b)
    assert sched.get_last_lr() == got[-1]


def test_scheduler_class_path_resolves_under_the_prefix_swap():
    import importlib

    mod, _, name = "neurosis.schedulers.LegacyCosineAnnealingWarmupRestarts".replace("neurosis.", "neurosis_amd.", 1).rpartition(".")
    cls = getattr(importlib.import_module(mod), name)
    opt = torch.optim.SGD(_groups([3e-5, 1.0, 1.0]), lr=1.0)
    sched = cls(opt, **SDXL_TE_SCHEDULER, verbose=False)
    assert [g["lr"] for g in opt.param_groups] == [3e-7, 3e-7, 3e-7]
    for _ in range(25):
        sched.step()
    assert [g["lr"] for g in opt.param_groups] == pytest.approx([3e-5, 1.0, 1.0], rel=1e-12)
    with pytest.raises(ValueError):
        cls(torch.optim.SGD(_groups([1.0]), lr=1.0), first_cycle_steps=5, warm_up_steps=5)


def _names(module, params):
    ids = {id(p) for p in params}
    return {n for n, p in module.named_parameters() if id(p) in ids}


def test_sdxl_te_embedders_train_what_their_outputs_depend_on():
    """CLIP-L under layer hidden / 11 trains everything but final_layer_norm; bigG under penultimate + pooled everything but logit_scale.
    Those two get no gradient from the step and stay out of the optimizer's groups."""
    from neurosis_amd.models.text_encoder.clip import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder2

    with torch.device("meta"):
        clip_l = FrozenCLIPEmbedder(device="meta", **SDXL_TE_CLIP_L)
        bigg = FrozenOpenCLIPEmbedder2(device="meta", **SDXL_TE_BIGG)
    assert clip_l.is_trainable and bigg.is_trainable and clip_l.base_lr == 1.0 and bigg.base_lr == 1.0
    assert all(p.requires_grad for p in clip_l.parameters()) and all(p.requires_grad for p in bigg.parameters())

    every = {n for n, _ in clip_l.named_parameters()}
    assert every - _names(clip_l, clip_l.trained_parameters()) == {"transformer.text_model.final_layer_norm.weight",
                                                                    "transformer.text_model.final_layer_norm.bias"}
    every = {n for n, _ in bigg.named_parameters()}
    assert every - _names(bigg, bigg.trained_parameters()) == {"model.logit_scale"}
    # registration order is kept (the flat store's layout)
    order = [n for n, _ in bigg.named_parameters()]
    trained = [n for n, p in bigg.named_parameters() if id(p) in {id(q) for q in bigg.trained_parameters()}]
    assert trained == [n for n in order if n in set(trained)]
    assert sum(p.numel() for p in bigg.trained_parameters()) + sum(p.numel() for p in clip_l.trained_parameters()) > 800_000_000


def test_trained_parameters_follow_the_selected_layer():
    from neurosis_amd.models.text_encoder.clip import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder2

    hf = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=4, num_attention_heads=1, vocab_size=100, max_position_embeddings=77)
    oc = dict(width=64, layers=4, heads=1, embed_dim=32, vocab_size=100)
    e = FrozenCLIPEmbedder(device="cpu", config=hf, layer="hidden", layer_idx=1, is_trainable=True)
    names = _names(e, e.trained_parameters())
    assert any(".layers.1." in n for n in names) and not any(".layers.2." in n for n in names) and not any("final_layer_norm" in n for n in names)
    e = FrozenCLIPEmbedder(device="cpu", config=hf, layer="last", is_trainable=True)
    assert _names(e, e.trained_parameters()) == {n for n, _ in e.named_parameters()}
    e = FrozenCLIPEmbedder(device="cpu", config=hf, layer="penultimate", always_return_pooled=True, is_trainable=True)
    assert _names(e, e.trained_parameters()) == {n for n, _ in e.named_parameters()}
    e = FrozenOpenCLIPEmbedder2(config=oc, device="cpu", layer="penultimate", is_trainable=True)
    names = _names(e, e.trained_parameters())
    assert not any(k in n for n in names for k in ("resblocks.3.", "ln_final", "text_projection", "logit_scale"))
    assert any("resblocks.2." in n for n in names) and "model.positional_embedding" in names
    e = FrozenOpenCLIPEmbedder2(config=oc, device="cpu", layer="last", is_trainable=True)
    names = _names(e, e.trained_parameters())
    assert any("resblocks.3." in n for n in names) and not any(k in n for n in names for k in ("ln_final", "text_projection", "logit_scale"))
    e = FrozenOpenCLIPEmbedder2(config=oc, device="cpu", layer="pooled", is_trainable=True)
    assert {n for n, _ in e.named_parameters()} - _names(e, e.trained_parameters()) == {"model.logit_scale"}


def test_trainable_embedders_refuse_what_their_chain_does_not_take():
    from neurosis_amd.models.text_encoder.clip import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder2

    hf = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, vocab_size=100)
    oc = dict(width=64, layers=2, heads=1, embed_dim=32, vocab_size=100)
    with pytest.raises(NotImplementedError, match="extended_chunks"):
        FrozenCLIPEmbedder(device="cpu", config=hf, is_trainable=True, extended_chunks=2)
    with pytest.raises(NotImplementedError, match="legacy"):
        FrozenOpenCLIPEmbedder2(config=oc, device="cpu", layer="penultimate", legacy=True, is_trainable=True)
    with pytest.raises(NotImplementedError, match="extended_chunks"):
        FrozenOpenCLIPEmbedder2(config=oc, device="cpu", is_trainable=True, extended_chunks=3)
    # frozen embedders keep accepting both
    FrozenCLIPEmbedder(device="cpu", config=hf, extended_chunks=2)
    FrozenOpenCLIPEmbedder2(config=oc, device="cpu", layer="penultimate", legacy=True)
    FrozenOpenCLIPEmbedder2(config=oc, device="cpu", extended_chunks=3)


def _engine(with_towers=True, **kw):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models.diffusion import DiffusionEngine
    from neurosis_amd.models.text_encoder.clip import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder2
    from neurosis_amd.modules.encoders.embedding import GeneralConditioner

    cfg = dict(in_channels=4, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[2], channel_mult=[1, 2], num_head_channels=16,
               use_linear_in_transformer=True, transformer_depth=1, context_dim=128, adm_in_channels=48, num_classes="sequential", use_checkpoint=False)
    clip_l = FrozenCLIPEmbedder(device="cpu", config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1),
                                layer="hidden", layer_idx=0, input_key="caption", is_trainable=with_towers, base_lr=1.0)
    bigg = FrozenOpenCLIPEmbedder2(config=dict(width=64, layers=2, heads=1, embed_dim=48), device="cpu", layer="penultimate", always_return_pooled=True,
                                   input_key="caption", is_trainable=with_towers, base_lr=0.5)
    return DiffusionEngine(D.UNetModel(**cfg), D.Denoiser(D.EpsPreconditioning()), None, conditioner=GeneralConditioner([clip_l, bigg]), **kw)


def test_engine_groups_one_per_trainable_embedder():
    """configure_optimizers builds the reference's groups (models/diffusion.py:261-296): "UNet", then one per trainable embedder with its
    name and initial_lr = base_lr, holding exactly the parameters that embedder trains"""
    seen = []
    eng = _engine(optimizer=lambda groups: seen.append(groups))
    with pytest.raises(TypeError):          # (the lambda is no fused optimizer: refused after the groups were built)
        eng.configure_optimizers()
    groups = seen[0]
    assert [g["name"] for g in groups] == ["UNet", "FrozenCLIPEmbedder", "FrozenOpenCLIPEmbedder2"]
    assert [g.get("initial_lr") for g in groups[1:]] == [1.0, 0.5]
    clip_l, bigg = eng.conditioner.embedders
    assert [id(p) for p in groups[1]["params"]] == [id(p) for p in clip_l.trained_parameters()]
    assert [id(p) for p in groups[2]["params"]] == [id(p) for p in bigg.trained_parameters()]
    assert id(bigg.model.logit_scale) not in {id(p) for g in groups for p in g["params"]}


def test_engine_refuses_what_the_trained_conditioner_step_does_not_take():
    eng = _engine()
    with pytest.raises(NotImplementedError, match="stream_optimizer"):
        eng.stream_optimizer = True
    frozen = _engine(with_towers=False)
    frozen.stream_optimizer = True          # (unchanged without trainable embedders)
    assert frozen.trainable_embedders() == []


def test_sdxl_te_config_instantiates_under_the_prefix_swap(monkeypatch):
    """configs/sdxl/sdxl-te.example.yaml's `model:` tree (tests/golden/config_class_paths_sdxl_te.json, make_golden_sdxl_te_config.py) built
    bottom-up on the meta device the way test_config_classpaths.py builds the other examples, with bitsandbytes.optim.AdamW8bit mapped to
    neurosis_amd.optimizers.AdamW8bit: both towers trainable, and configure_optimizers gives the reference's groups and the scheduler"""
    import tests.test_config_classpaths as T
    from neurosis_amd.optimizers import AdamW8bit
    from neurosis_amd.schedulers import LegacyCosineAnnealingWarmupRestarts

    nodes = json.loads((G / "config_class_paths_sdxl_te.json").read_text())["configs/sdxl/sdxl-te.example.yaml"]["nodes"]
    base_swap = T.swap
    monkeypatch.setattr(T, "swap", lambda cp: "neurosis_amd.optimizers.AdamW8bit" if cp == "bitsandbytes.optim.AdamW8bit" else base_swap(cp))
    base_coerce = T.coerce

    def coerce(cls, kwargs):
        # (jsonargparse also reads `3e-7` -- a string to YAML 1.1 -- as a float where the hint is a union with float: the scheduler's min_lr)
        import inspect

        hints = {n: p.annotation for n, p in inspect.signature(cls.__init__).parameters.items()}
        kwargs = {k: (float(v) if isinstance(v, str) and str(hints.get(k, "")).startswith("float |") else v) for k, v in kwargs.items()}
        return base_coerce(cls, kwargs)

    monkeypatch.setattr(T, "coerce", coerce)
    for node in nodes:
        assert node["resolves_in_reference"] or node["class_path"] in T.BROKEN_IN_REFERENCE, node["class_path"]
        T.resolve(T.swap(node["class_path"]))
    eng = T.build(nodes, "model")
    assert [type(e).__name__ for e in eng.trainable_embedders()] == ["FrozenCLIPEmbedder", "FrozenOpenCLIPEmbedder2"]
    out = eng.configure_optimizers()
    opt, sched = out["optimizer"], out["lr_scheduler"]["scheduler"]
    assert isinstance(opt, AdamW8bit) and isinstance(sched, LegacyCosineAnnealingWarmupRestarts)
    assert [g["name"] for g in opt.param_groups] == ["UNet", "FrozenCLIPEmbedder", "FrozenOpenCLIPEmbedder2"]
    assert [g.get("initial_lr") for g in opt.param_groups[1:]] == [1.0, 1.0]
    assert opt.param_groups[0]["lr"] == pytest.approx(3e-7) and opt.defaults["lr"] == pytest.approx(3e-5)
